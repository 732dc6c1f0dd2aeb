// Body of the backward — included by iql_bwd_kernel and iql_bwd_group_kernel (iqlhip_kernels.h):
// ONE body for the single-agent kernel and its trainer-group form, so the arithmetic exists once.  blockIdx.x / gridDim.x
// are the block's index and grid size of ONE agent's launch in both (a group kernel's agent is blockIdx.y).
// In scope: template flags BF16, FULL, MULTI, the leading arguments q_*, `p` (StepParams) and KPF (the un-waited
// argument-line prefetch, which reads the kernel-argument block itself: iql_bwd_kernel only).
// RW (iql_bwd_rw_kernel only; elsewhere false, and rw_w / rw_td null constants): per-row loss weights rw_w[row] and the
// optional TD-error output rw_td[row][2].
  RT_ENTRY();
  const int bid = blockIdx.x;
  const int x = bid & 7;
  const int h_S = (int)(q_dims & 255u), h_A = (int)((q_dims >> 8) & 63u), h_pol = (int)((q_dims >> 14) & 1u);
  const int h_ld = (int)(q_ldB & 1023u), h_rows = (int)(q_ldB >> 10);
  const int h_MB = (int)(q_mbc & 0xFFFFu), n_chunk = (int)(q_mbc >> 16);
  const int n_rt = (int)(q_rts & 1023u), h_spb = (int)(q_rts >> 10);
  // Touch every 64-byte line of `p` this block will read, NOW and without waiting (one-slice instantiations only): the
  // fetch in PIN_REST() below then finds the lines on their way — hipcc splits it into three to four dependent groups,
  // each a scalar-cache miss of its own otherwise (interleaved A/B with the deferred fetch: backward 8.53 -> 8.29 us).
  // hipcc does not see that an asm's scalar loads complete late, so the destination registers stay allocated — as
  // operands of the waiting asm in PIN_REST() — until that wait, and the instantiations that do this must not spill
  // SGPRs (a spilled destination's register is handed to a live value at once: the late write then corrupts it — a memory
  // fault at 600 rows when the MULTI instantiations still did it); __graft_entry__.build() fails the build otherwise.
  unsigned kpf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (!MULTI && KPF) {
    const unsigned long long ka = (unsigned long long)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr unsigned KA_P = 56;       // `p` follows five pointers and four words in the argument block
    const unsigned o_net = KA_P + (unsigned)offsetof(StepParams, net) + (unsigned)sizeof(NetPtrs) * (unsigned)(x & 3);
    const unsigned o_go = KA_P + (unsigned)offsetof(StepParams, go) + (unsigned)sizeof(NetGrad) * (unsigned)(x & 3);
    const unsigned o_t0 = (KA_P + (unsigned)offsetof(StepParams, log_std)) & ~63u;
    static_assert(KA_P + sizeof(StepParams) - ((KA_P + offsetof(StepParams, log_std)) & ~(size_t)63) <= 256, "kernel-argument tail: more than 4 lines");
    unsigned d0, d1, d2, d3, d4, d5, d6, d7;
    asm volatile(
        "s_load_dword %0, %8, %9\n\ts_load_dword %1, %8, %10\n\ts_load_dword %2, %8, %11\n\t"
        "s_load_dword %3, %8, %12\n\ts_load_dword %4, %8, %13\n\ts_load_dword %5, %8, %14\n\t"
        "s_load_dword %6, %8, %15\n\ts_load_dword %7, %8, %16"
        : "=&s"(d0), "=&s"(d1), "=&s"(d2), "=&s"(d3), "=&s"(d4), "=&s"(d5), "=&s"(d6), "=&s"(d7)
        : "s"(ka), "s"(o_net), "s"(o_net + (unsigned)sizeof(NetPtrs) - 4u), "s"(o_go), "s"(o_go + (unsigned)sizeof(NetGrad) - 4u),
          "s"(o_t0), "s"(o_t0 + 64u), "s"(o_t0 + 128u), "s"(o_t0 + 192u));
    kpf[0] = d0; kpf[1] = d1; kpf[2] = d2; kpf[3] = d3; kpf[4] = d4; kpf[5] = d5; kpf[6] = d6; kpf[7] = d7;
  }
  // A net's blocks stay on two XCDs (net = x & 3: its weights and activations live in those two L2s; rotating the nets
  // over all XCDs made multi-round launches 5-8 % SLOWER).  But the policy's blocks are 1.5-2.5x as long as the scalar
  // nets', and in a multi-round launch XCDs 3 and 7 finished at 33 us while the other six idled from 17 us on (obs 39 /
  // act 28, 1 024 rows, bf16).  MULTI: the policy's LAST n_don dW1-tile blocks are therefore moved to the FRONT of the
  // other six XCDs' queues (the first ceil(n_don / 6) grid rows; host: launch_bwd) — long blocks first: at the ends of
  // those queues they started at 22 us and finished at 36; their old slots return at once.
  const int n_a = 32 * n_chunk;
  const int bsl2 = MULTI ? ((h_spb >> 2) & 3) : 0;     // (b) blocks: log2 of the column slices per block
  const int n_b = (4 >> bsl2) * n_rt;
  int net = x & 3;
  int local_ = (bid >> 3) * 2 + (x >> 2);
  if (MULTI) {
    const int n_don = h_spb >> 8;
    const int n_e = (n_don + 5) / 6;
    const int q = bid >> 3;
    if (q < n_e) {
      const int j = q * 6 + (x - (x >> 2));       // x in {0,1,2,4,5,6} -> 0..5
      if (net == IQLHIP_NET_PI || j >= n_don) return;
      net = IQLHIP_NET_PI;
      local_ = n_a + n_b - n_don + j;
    } else {
      local_ -= 2 * n_e;
      if (net == IQLHIP_NET_PI && local_ >= n_a + n_b - n_don) return;
    }
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int B = h_rows;
  const int MB = h_MB;
  const ArenaOff ao = arena_off(net, h_S, h_A, h_pol == IQLHIP_POLICY_GAUSSIAN);

  const NetPtrs np = p.net[net];
  const NetGrad go = p.go[net];
  const int D = ao.d;
  const int Dp = (D + 15) & ~15;      // 16 or 32
  const int DYLD = Dp + 4;            // dY row stride in LDS: 16-B aligned rows (float4 reads of a row's dims)
  const float* w2 = q_params + ao.w2;
  // (bf16 path: H0 / H1 are stored as bf16 — the same element offsets, half the bytes; the pointers below then carry
  //  the bf16 arrays' addresses and are only ever dereferenced through ld4 / ld2)
  const float* H1g = BF16 ? (const float*)((const __bf16*)q_h1 + net * MB * HID) : q_h1 + net * MB * HID;
  const float* H0g = BF16 ? (const float*)((const __bf16*)q_h0 + net * MB * HID) : q_h0 + net * MB * HID;
  // Everything the block still needs from the by-value StepParams is fetched by PIN_REST(), which each branch invokes
  // right BEHIND the issue of its first global loads: those depend on preloaded arguments only, so the ~500-cycle fetch
  // of the argument block now runs under their latency instead of in front of them (one batch of scalar loads behind
  // one wait; in the one-slice instantiations the lines were touched at the top and the prefetch registers' live range
  // ends at the wait below, which is free by then).
#define PIN_REST()                                                                                                          \
  do {                                                                                                                      \
    float* sa_ = p.sc.slab_a; float* sb_ = p.sc.slab_b;                                                                     \
    const long long sbo_ = p.sc.slab_b_off[net], npar_ = p.n_params;                                                        \
    PIN_P(np.w1); PIN_P(sa_); PIN_P(sb_);                                                                                   \
    PIN_S(sbo_); PIN_S(npar_); PIN_S(go.w1); PIN_S(go.b1); PIN_S(go.w2); PIN_S(go.b2); PIN_S(go.log_std);                   \
    PIN_S(p.inv_batch); PIN_S(p.hy.iql_tau); PIN_S(p.hy.beta); PIN_S(p.hy.discount); PIN_S(p.hy.exp_adv_max);               \
    if constexpr (!MULTI && KPF)                                                                                            \
      asm volatile("s_waitcnt lgkmcnt(0)" ::"s"(kpf[0]), "s"(kpf[1]), "s"(kpf[2]), "s"(kpf[3]), "s"(kpf[4]), "s"(kpf[5]),   \
                   "s"(kpf[6]), "s"(kpf[7]));                                                                               \
  } while (0)
  if (local_ >= n_a + n_b) return;
  // MULTI: the (b) blocks walk 2 / 4 slices and run 2-3x as long as a dW1 tile — they take the FIRST block indices so
  // that the launch ends on short blocks (longest first); one-slice grids keep the dW1 tiles first
  const int local = MULTI ? ((local_ < n_b) ? n_a + local_ : local_ - n_b) : local_;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  STAMP_BASE(p, 2048 * 16);   // second half of the stamp buffer: the forward kernel owns the first
  STAMP(p, 0);

  if (local < n_a) {
    // ===================== (a): dW1[j-tile][i-tile] over one 256-row chunk =====================
    const int c = local >> 5;
    const int jt = (local >> 2) & 7;
    const int it = local & 3;
    const int j0 = jt * 32, i0 = it * 64;
    const int cbase = c * CHUNK_ROWS;
    float* red = smem;                               // [4][32][T64_LD]
    const int DYA = Dp + 4;                          // row stride of dYs / dLs here: 16-B aligned rows (float4 reads)
    float* dYs = red + 4 * 32 * T64_LD;              // [256][DYA]
    float* dLs = dYs + CHUNK_ROWS * DYA;            // [256][DYA]  (gaussian pi designated block only)
    float* W2s = dLs + CHUNK_ROWS * DYA;            // [D][32]
    float* rsm = W2s + 32 * 32;                      // [64] small reductions
    float* wS = rsm + 64;                            // [256] policy: per-row advantage weight
    const bool designated = (jt == 0 && it == 2);    // db2 and dlog_std: a block without other extras
    const bool loss_block = (jt == 1 && it == 2);    // the loss sums: another one
    // the column-independent extras of this j tile: db1 by the it == 0 block; dW2 by the it == 0 block when D == 1
    // (two fmas per row) but, when D > 1 (policy: MFMAs and an LDS round trip), one half of the j columns each by
    // the it == 1 and it == 3 blocks — all on one block made that block the last to finish in the whole kernel
    const bool do_db1 = (it == 0);
    const bool do_dw2 = (D == 1) ? (it == 0) : (it == 1 || it == 3);
    const int tb_own = (it == 3) ? 1 : 0;            // D > 1: which of a lane's two j columns this block's dW2 covers
    const bool extras = do_db1 || do_dw2;

    // ---- loads, in the order they are needed (vmcnt retires in issue order): the per-row loss
    // inputs first, then the 96 KiB of activation tiles, which stream in under the dY arithmetic.
    const int prow = cbase + tid;
    RowIn in;
    const float lsr = pi_ls_issue_hot(q_params + ao.log_std, q_xb, h_pol, h_A);
    const bool is_pi = (net == IQLHIP_NET_PI);
    row_issue_hot(q_heads, q_xb, h_ld, h_S, h_A, BROW(prow), in);           // scalar partials, r, d (the policy needs h[1..3] for w)
    float rwc = 1.f;                                                        // RW: this row's loss weight
    if constexpr (RW) rwc = rw_w[(unsigned)BROW(prow)];
    // Policy: its per-(row, dim) inputs are loaded as (row, dim) work items — thread (r8 = tid >> 3, sub = tid & 7)
    // takes rows r8 + 32c, c = 0..7, and action dim sub (+ 8e) — so that one load instruction touches 6-8 cache
    // lines.  With thread = row every such load touched 48-64 lines; the 16 of them held the load queue for 8.5 k
    // cycles and made the policy's (a) blocks (10-13 us) the long pole of the whole kernel (others: 6-9 us).
    const int r8 = tid >> 3, sub = tid & 7;
    const f32x4* hpb = (const f32x4*)(q_heads + MB * HEAD_LD);
    const float* hpf = q_heads + MB * HEAD_LD;
    const float* xbp = q_xb;
    f32x4 php[8];
    float pac[8];
    if (is_pi) {
      const unsigned dd0 = (unsigned)min(sub, h_A - 1);
      const unsigned uA = (unsigned)h_A, uld = (unsigned)h_ld, uS = (unsigned)h_S;
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) {
        const unsigned rowc = (unsigned)BROW(cbase + r8 + 32 * cc);
        php[cc] = *(const f32x4*)(hpf + 4u * (rowc * uA + dd0));
        pac[cc] = xbp[rowc * uld + uS + dd0];
      }
    }
    float w2pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ec = min(tid + 256 * q, D * 32 - 1);      // clamped: unconditional load
      w2pre[q] = w2[(unsigned)((ec >> 5) * HID + j0 + (ec & 31))];
    }
    // wave w reduces its 64 rows, 4 per MFMA: instruction ks of lane group g takes row AROW(ks) = 64w + 16(ks>>2) +
    // 4g + (ks&3) — the row a lane's accumulator register (ks&3) of the 16-row tile (ks>>2) holds when dH1 itself
    // comes out of an MFMA (wide heads, below), so that result feeds the dW1 MFMA without a shuffle.  Rows >= B are
    // clamped to a valid row: their dY is 0, so they contribute nothing.
#define AROW(ks) (64 * wave + 16 * ((ks) >> 2) + 4 * g + ((ks) & 3))
    typename Frag2<BF16>::type hh[16];
    typename Frag4<BF16>::type bb[16];
    // The 96 KB of activation tiles are requested in four groups with the chunk's loss arithmetic BETWEEN them: a wave spends
    // ~4 k cycles just issuing its ~60 loads (the four waves share the CU's one vector-memory pipe, ~64 cycles per 1 KB
    // instruction) with the vector ALU idle, and the per-row inputs requested first are back after the first third of that —
    // the policy's 2.7 k cycles of advantage weights and (row, dim) terms, which made its blocks the kernel's last, now run
    // inside the issue phase instead of behind it.  (Scheduling barriers: hipcc otherwise gathers all loads in front again.)
#define HB_LOAD(k0_, k1_)                                                                               \
    _Pragma("unroll") for (int ks = (k0_); ks < (k1_); ++ks) {                                          \
      const unsigned row = (unsigned)BROW(cbase + AROW(ks));                                            \
      hh[ks] = ld2<BF16>(H1g, row * (unsigned)HID + (unsigned)(j0 + 2 * l15));                          \
      bb[ks] = ld4<BF16>(H0g, row * (unsigned)HID + (unsigned)(i0 + 4 * l15));                          \
    }
    HB_LOAD(0, 4);
    PIN_REST();
    float* slab = p.sc.slab_a + (long long)c * p.n_params;
    // dropout: the saved activations are post-dropout, so (h > 0) already encodes relu AND keep; the chain
    // rule only adds the 1/(1-p) multiplier
    const float dscale = (net == IQLHIP_NET_PI && p.drop_bits != nullptr) ? p.drop_scale : 1.f;
    STAMP(p, 10);
    // ---- dY for the 256 rows of the chunk (thread = row)
    {
      const int row = prow;
#pragma unroll
      for (int q = 0; q < 4; ++q) {           // [Dp][32], zero rows beyond D (operand of the dH1 MFMA)
        const int e = tid + 256 * q;
        if (e < Dp * 32) W2s[e] = (e < D * 32) ? w2pre[q] : 0.f;
      }
      float lossA = 0.f, lossB = 0.f;
      const PiConst pc = pi_consts_hot(p, h_pol, net, lsr);
      if (!is_pi) {
        float* dyrow = dYs + tid * DYA;
        for (int dd = 0; dd < Dp; ++dd) dyrow[dd] = 0.f;
        if constexpr (RW) {
          // the finished unweighted values times the row's weight, last: a weight of 1.0f leaves their bits
          if (row < B) {
            float dy0;
            row_finish(p, net, in, &dy0, lossA, lossB);
            dyrow[0] = dy0 * rwc;
            lossA *= rwc;
            lossB *= rwc;
            // the chunk's Q1 loss block owns the TD errors of its 256 rows (thread = row)
            if (rw_td != nullptr && loss_block && net == IQLHIP_NET_Q1) *(f32x2*)(rw_td + 2u * (unsigned)row) = row_td_errors(p, in);
          }
        } else {
          if (row < B) row_finish(p, net, in, dyrow, lossA, lossB);
        }
      } else {
        // phase 1 (thread = row): the advantage weight (iql.py:519); rows >= B get w = 0, hence dY = 0
        float wrow = 0.f;
        if (row < B) {
          const float tq = fminf(sum4(in.h[2]), sum4(in.h[3]));
          const float u = tq - sum4(in.h[1]);
          wrow = fminf(expf(p.hy.beta * u), p.hy.exp_adv_max);
          if constexpr (RW) wrow *= rwc;       // feeds pi_items8, the log_std gradient and the actor loss sum
        }
        STAMP(p, 5);
        wS[tid] = wrow;
      }
      __builtin_amdgcn_sched_barrier(0);
      HB_LOAD(4, 8);
      __builtin_amdgcn_sched_barrier(0);
      const bool gauss = (h_pol == IQLHIP_POLICY_GAUSSIAN);
      const bool want_dls = designated && gauss;
      float wv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (is_pi) {
        __syncthreads();                       // (net is block-uniform)
        STAMP(p, 6);
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) wv[cc] = wS[r8 + 32 * cc];
      }
      __builtin_amdgcn_sched_barrier(0);
      HB_LOAD(8, 12);
      __builtin_amdgcn_sched_barrier(0);
      if (is_pi) {
        // phase 2 (thread = (row, dim)): mean, log-prob term, dL/dpre and dL/dlog_std of every (row, dim) — eight
        // rows of one dim per thread and group of 8 dims, as straight-line select code (pi_items8): written with
        // per-item branches this phase was ~110 LDS / branch round trips (3.3 k cycles, the policy blocks' long pole)
        const int A = h_A;
        const float invB = p.inv_batch;
        const int DpZ = (D <= 8) ? 8 : Dp;      // dims the dH1 / dW2 products read as operands (zero-filled beyond A)
        for (int e = 0; 8 * e < DpZ; ++e) {
          const int dd = sub + 8 * e;
          float dyv[8], dlv[8];
#pragma unroll
          for (int cc = 0; cc < 8; ++cc) { dyv[cc] = 0.f; dlv[cc] = 0.f; }
          if (8 * e < A) {                     // (block-uniform; groups beyond A are padding up to Dp: zeros, no loads)
            const int ddc = min(dd, A - 1);
            const float ivar = __shfl(pc.ivar, ddc);     // lane ddc holds dim ddc's constants; the whole wave is here
            const float ls = __shfl(pc.ls, ddc);
            if (e == 0) {
              pi_items8(php, pac, wv, dd < A, gauss, ivar, ls, invB, dyv, dlv, lossA);
            } else {                           // action dims >= 8 (wide action spaces): loaded here, 8 at a time
              f32x4 hv[8];
              float acv[8];
#pragma unroll
              for (int cc = 0; cc < 8; ++cc) {
                const unsigned rowc = (unsigned)BROW(cbase + r8 + 32 * cc);
                hv[cc] = *(const f32x4*)(hpf + 4u * (rowc * (unsigned)A + (unsigned)ddc));
                acv[cc] = xbp[rowc * (unsigned)h_ld + (unsigned)(h_S + ddc)];
              }
              pi_items8(hv, acv, wv, dd < A, gauss, ivar, ls, invB, dyv, dlv, lossA);
            }
          }
#pragma unroll
          for (int cc = 0; cc < 8; ++cc) dYs[(r8 + 32 * cc) * DYA + dd] = dyv[cc];
          if (want_dls) {
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) dLs[(r8 + 32 * cc) * DYA + dd] = dlv[cc];
          }
        }
        STAMP(p, 7);
      }
      __builtin_amdgcn_sched_barrier(0);
      HB_LOAD(12, 16);
      __builtin_amdgcn_sched_barrier(0);
#undef HB_LOAD
      STAMP(p, 11);
      if (loss_block) {
        const float sA = block_sum_256(lossA, rsm);
        if (net == IQLHIP_NET_V && tid == 0) p.sc.loss_parts[0 * 64 + c] = sA;
        if (net == IQLHIP_NET_PI && tid == 0) p.sc.loss_parts[3 * 64 + c] = sA;
        if (net == IQLHIP_NET_Q1) {
          const float sB = block_sum_256(lossB, rsm + 8);
          if (tid == 0) { p.sc.loss_parts[1 * 64 + c] = sA; p.sc.loss_parts[2 * 64 + c] = sB; }
        }
      }
    }
    __syncthreads();
    STAMP(p, 1);
    if (designated && D > 8) {
      // db2[dd] = sum_r dY[r][dd];  dlog_std[dd] = sum_r w (1 - diff^2/var) * inv_batch (inside clamp range only).
      // Wide heads: thread (dim tid & 31, row group tid >> 5) sums 32 rows, the 8 partial sums meet in LDS (the
      // tile-reduction buffer is idle until after the MFMA phase; only wave 0's part of it is touched here).  A
      // dim per wave and iteration, each with its own load and store, took ~1.4 k cycles per dim: 9.7 k at D = 28
      // (for D <= 8 that loop, at most two dims per wave, is the cheaper one and stays).
      const bool gls = (net == IQLHIP_NET_PI && h_pol == IQLHIP_POLICY_GAUSSIAN);
      const int dd = tid & 31, rg = tid >> 5;
      float s = 0.f, sl = 0.f;
      if (dd < D) {
#pragma unroll 8
        for (int r = 0; r < 32; ++r) {
          s += dYs[(rg * 32 + r) * DYA + dd];
          if (gls) sl += dLs[(rg * 32 + r) * DYA + dd];
        }
      }
      red[rg * 64 + dd] = s;
      red[rg * 64 + 32 + dd] = sl;
      __syncthreads();                 // (block-uniform condition)
      if (tid < D) {
        float ts = 0.f, tl = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { ts += red[k * 64 + tid]; tl += red[k * 64 + 32 + tid]; }
        slab[go.b2 + tid] = ts;
        if (gls) {     // (lsr: this lane's raw log_std, loaded at the top of the block — tid < D <= 32 is lane tid of wave 0;
                       //  a load issued HERE would queue behind the whole activation-tile stream)
          const bool inside = (lsr >= p.hy.log_std_min) && (lsr <= p.hy.log_std_max);
          slab[go.log_std + tid] = inside ? tl * p.inv_batch : 0.f;
        }
      }
    } else if (designated && net != IQLHIP_NET_PI) {
      // scalar heads (V, Q1, Q2; D = 1): one 256-term sum by wave 0 — 4 rows per lane, then a shuffle tree.  (Kept as it is:
      // these blocks are not the kernel's last ones, and db2 of a Q net, sum_r (q - y) / B, cancels so heavily that
      // ANY other summation order moves it by ~2e-5 of itself against the reference's equally arbitrary order.)
      if (wave == 0) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) s += dYs[(lane + 64 * q) * DYA];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) slab[go.b2] = s;
      }
    } else if (designated) {
      // the policy with D <= 8: thread (dim tid & 7, row group tid >> 3) sums 8 rows, the 32 partial sums per dim meet in LDS and are
      // added in row-group order by one thread per dim (a dim per wave and pass, with a 6-level shuffle tree per dim,
      // took 2.9 k cycles on the one block that does this — the last block of the whole kernel)
      const bool gls = (net == IQLHIP_NET_PI && h_pol == IQLHIP_POLICY_GAUSSIAN);
      const int dd = tid & 7, rg = tid >> 3;
      // (both stages are balanced trees: these sums cancel heavily — db2 of a Q net is sum_r (q - y) / B — and a
      //  sequential 256-term sum lost a digit against the reference: 2.1e-5 instead of 2.6e-6 on one fixture)
      float s = 0.f, sl = 0.f;
      if (dd < D) {
        float a[8], b[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          a[r] = dYs[(rg * 8 + r) * DYA + dd];
          b[r] = gls ? dLs[(rg * 8 + r) * DYA + dd] : 0.f;
        }
        s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        sl = ((b[0] + b[1]) + (b[2] + b[3])) + ((b[4] + b[5]) + (b[6] + b[7]));
      }
      red[rg * 16 + dd] = s;
      red[rg * 16 + 8 + dd] = sl;
      __syncthreads();                 // (block-uniform condition)
      if (tid < D) {
        float u[32], w[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) { u[k] = red[k * 16 + tid]; w[k] = red[k * 16 + 8 + tid]; }
#pragma unroll
        for (int st = 16; st > 0; st >>= 1) {
#pragma unroll
          for (int k = 0; k < 16; ++k) if (k < st) { u[k] += u[k + st]; w[k] += w[k + st]; }
        }
        const float ts = u[0], tl = w[0];
        slab[go.b2 + tid] = ts;
        if (gls) {
          const bool inside = (lsr >= p.hy.log_std_min) && (lsr <= p.hy.log_std_max);
          slab[go.log_std + tid] = inside ? tl * p.inv_batch : 0.f;
        }
      }
    }
    STAMP(p, 2);

    // ---- operand phase: A values av[ks][ta] = dH1[row][j0 + 2*l15 + ta] from registers + LDS
    float av[16][2];
    float db1a[2] = {0.f, 0.f};
    float dw2a[2] = {0.f, 0.f};    // D == 1
    if (D == 1) {
      const float w2a = W2s[2 * l15], w2b = W2s[2 * l15 + 1];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const float dy = dYs[AROW(ks) * DYA];
        av[ks][0] = ((float)hh[ks][0] > 0.f) ? dy * w2a * dscale : 0.f;
        av[ks][1] = ((float)hh[ks][1] > 0.f) ? dy * w2b * dscale : 0.f;
        if (do_dw2) {
          dw2a[0] = fmaf(dy, (float)hh[ks][0], dw2a[0]);
          dw2a[1] = fmaf(dy, (float)hh[ks][1], dw2a[1]);
        }
      }
    } else {
      // wide heads (policy): dH1pre[row][j] = sum_dd dY[row][dd] W2[dd][j] on the matrix cores — per wave 4 row
      // tiles x 2 j tiles x Dp/4 k-steps (32 or 64 MFMAs) instead of 2 D fmas per (row, j) on the vector ALU (1 024
      // per thread at D = 28).  A = dY (m = row 16t + l15, k = dd), B = W2 (k = dd, n = j = 2 l15 + ta, zero rows
      // beyond D); lane (g, l15) gets rows 16t + 4g + reg = AROW(4t + reg): its own operand rows of the dW1 MFMA.
      // fp32 MFMA is an exact fma chain over k, i.e. the same sum in the same dim order as the scalar code.
      f32x4 pre[4][2];
#pragma unroll
      for (int t = 0; t < 4; ++t) { pre[t][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; pre[t][1] = pre[t][0]; }
      // k-steps of 4 action dims, rounded up to 2 / 4 / 8 (dims 4 NK .. are zero operands: not multiplied at all)
      if (D <= 8) dh1_mfma<2>(pre, dYs, W2s, DYA, wave, g, l15);
      else if (D <= 16) dh1_mfma<4>(pre, dYs, W2s, DYA, wave, g, l15);
      else dh1_mfma<8>(pre, dYs, W2s, DYA, wave, g, l15);
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        av[ks][0] = ((float)hh[ks][0] > 0.f) ? pre[ks >> 2][0][ks & 3] * dscale : 0.f;
        av[ks][1] = ((float)hh[ks][1] > 0.f) ? pre[ks >> 2][1][ks & 3] * dscale : 0.f;
      }
    }
    if (do_db1) {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) { db1a[0] += av[ks][0]; db1a[1] += av[ks][1]; }
    }

    // ---- MFMA phase
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (BF16) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {       // rows (k) 8q..8q+7 of this lane's 16
        bf16x8 A[2], Bv[4];
#pragma unroll
        for (int ta = 0; ta < 2; ++ta) {
          float t8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) t8[e] = av[8 * q + e][ta];
          A[ta] = pack8s(t8);
        }
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) {      // (H0 arrives as bf16: the operand is assembled, not converted)
#pragma unroll
          for (int e = 0; e < 8; ++e) Bv[tb][e] = bb[8 * q + e][tb];
        }
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
          for (int tb = 0; tb < 4; ++tb) acc[ta][tb] = MFMA_BF16(A[ta], Bv[tb], acc[ta][tb]);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
          for (int tb = 0; tb < 4; ++tb) acc[ta][tb] = MFMA16(av[ks][ta], bb[ks][tb], acc[ta][tb]);
      }
    }
    f32x4 acc2[2][2];   // dW2 tiles [dt][tb] (MFMA path, D > 1, extras blocks only)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc2[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int ndt = Dp >> 4;
    if (do_dw2 && D > 1) {
      // all 16 LDS operands first, then the MFMAs (a read under a per-iteration `if` was waited for on the spot:
      // 16 exposed LDS latencies made these blocks the last of the kernel)
      float ad[16];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) ad[ks] = dYs[AROW(ks) * DYA + l15];
      float hsel[16];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) hsel[ks] = tb_own ? (float)hh[ks][1] : (float)hh[ks][0];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) acc2[0][0] = MFMA16(ad[ks], hsel[ks], acc2[0][0]);
      if (ndt > 1) {
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) ad[ks] = dYs[AROW(ks) * DYA + 16 + l15];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) acc2[1][0] = MFMA16(ad[ks], hsel[ks], acc2[1][0]);
      }
    }
    STAMP(p, 3);

    // ---- cross-wave reduction of the 32x64 tile through LDS, then coalesced store.  The extras (db1 / dW2 partial
    // sums of the 4 waves) are staged in the same pass, in the dLs region — only the loss-sum block (it == 2), which
    // has no extras, ever uses that region — so one barrier serves both reductions.
    // exA [4 waves x 4 lane groups][2 rows: db1, scalar dW2][32 cols]: every lane stores its own partial sums — the
    // sums over the lane groups g and over the waves are formed after the barrier, in the order ((g0+g1)+(g2+g3)) per
    // wave, ((w0+w1)+(w2+w3)) over the waves, i.e. the sums the two shuffle steps per value used to form before the
    // barrier (4 values x 2 dependent cross-lane steps: ~1.2 k cycles of every block that owns extras).
    // exB [4 waves][Dp rows][32 cols]: the MFMA tiles of a wide head's dW2.
    float* exA = dLs;
    float* exB = dLs + 1024;
    {
      float* myred = red + wave * 32 * T64_LD;
#pragma unroll
      for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int jl = 2 * (4 * g + reg) + ta;
          f32x4 v = (f32x4){acc[ta][0][reg], acc[ta][1][reg], acc[ta][2][reg], acc[ta][3][reg]};
          *(f32x4*)(myred + jl * T64_LD + 4 * l15) = v;
        }
    }
    if (extras) {
      float* mine = exA + (wave * 4 + g) * 64 + 2 * l15;
      *(f32x2*)mine = (f32x2){db1a[0], db1a[1]};
      if (D == 1) *(f32x2*)(mine + 32) = (f32x2){dw2a[0], dw2a[1]};
      if (D > 1 && do_dw2) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          if (dt < ndt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
              exB[(wave * 32 + 16 * dt + 4 * g + reg) * 32 + 2 * l15 + tb_own] = acc2[dt][0][reg];
      }
    }
    __syncthreads();
    {
      float* gw1 = slab + go.w1;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int f = tid + 256 * q;
        const int jl = f >> 4, i4 = f & 15;
        f32x4 s = *(const f32x4*)(red + jl * T64_LD + 4 * i4);
#pragma unroll
        for (int w = 1; w < 4; ++w) s += *(const f32x4*)(red + w * 32 * T64_LD + jl * T64_LD + 4 * i4);
        *(f32x4*)(gw1 + (j0 + jl) * HID + i0 + 4 * i4) = s;
      }
    }
    if (extras) {
      // (only the rows this block stores: row 0 = db1 costs 16 LDS reads per value, and a wave that holds row-0 AND row-1
      //  lanes runs both paths one after the other — 790 cycles at the end of the policy's dW2 blocks, the kernel's last
      //  blocks, which do not even own db1)
      const int e_lo = do_db1 ? 0 : 32;
      const int e_hi = do_dw2 ? (1 + D) * 32 : 32;
      for (int e = tid + e_lo; e < e_hi; e += 256) {
        const int rr = e >> 5, jj = e & 31;
        float s;
        if (rr == 0 || D == 1) {
          float wsum[4];
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const float* a = exA + (w * 4) * 64 + rr * 32 + jj;
            wsum[w] = (a[0] + a[64]) + (a[128] + a[192]);
          }
          s = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        } else {
          const float* b = exB + (rr - 1) * 32 + jj;
          s = (b[0] + b[1024]) + (b[2048] + b[3072]);
        }
        if (rr == 0) { if (do_db1) slab[go.b1 + j0 + jj] = s; }
        else if (do_dw2 && (D == 1 || (jj & 1) == tb_own)) slab[go.w2 + (rr - 1) * HID + j0 + jj] = s;
      }
    }
    STAMP(p, 4);
    RT_STAMP(p, 14, rt_entry_);
    RT_STAMP(p, 15, iql_realtime());
    return;
  }
#undef AROW

  // ===================== (b): dH0 / dW0 / db0 for one 32-row tile and 64-column slice =====================
  {
    const int lb = local - n_a;
    const int rt = lb >> (2 - bsl2);
    int i0 = ((lb & ((4 >> bsl2) - 1)) << bsl2) * 64;      // first (or only) column slice of this block
    const int row0 = rt * RT_ROWS;
    const int k0 = ao.k0;
    const int ld = h_ld;
    const int xoff = 0;                   // trainable nets read s or [s|a]: both start at column 0
    const float* w1 = np.w1;

    float* dH1s = smem;                              // [32][H0_LD]  (bf16 path: the same tile as bf16 [32][H0B_LD], below)
    __bf16* dH1b = (__bf16*)smem;
    float* red = dH1s + RT_ROWS * H0_LD;             // [4][32][T64_LD]
    float* dH0s = red + 4 * 32 * T64_LD;             // [32][T64_LD]
    float* dYs = dH0s + RT_ROWS * T64_LD;            // [32][DYLD]
    float* Xr = dYs + RT_ROWS * 36;                  // [32][ld] packed rows (parked late); 16-B aligned

    // ---- issue every global load of the block, first-needed first (vmcnt retires in issue order)
    RowIn in;
    const int prow = BROW(row0 + (tid & 31));
    const float lsr = pi_ls_issue_hot(q_params + ao.log_std, q_xb, h_pol, h_A);
    // the scalar nets' per-row loss inputs are consumed by the first 32 threads only: wave 0 alone loads them
    // (these loads head the in-order queue — issued by all four waves they delayed every load behind them);
    // the policy's own inputs follow below
#pragma unroll
    for (int i = 0; i < 6; ++i) in.h[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    in.r = 0.f; in.d = 0.f;
    if (wave == 0 && net != IQLHIP_NET_PI) row_issue_hot(q_heads, q_xb, h_ld, h_S, h_A, prow, in);
    float rwc = 1.f;                      // RW: the loss weight of the row this thread forms dY for
    if constexpr (RW) {
      if (net != IQLHIP_NET_PI) { if (wave == 0) rwc = rw_w[(unsigned)prow]; }
      else rwc = rw_w[(unsigned)BROW(row0 + (tid >> 3))];
    }
    // policy: the loss arithmetic of the 32 rows is spread over all 256 threads — thread (row tid>>3,
    // dims (tid&7) + 8c) — instead of 32 threads walking all dims while 224 wait at the barrier
    const int prl = tid >> 3, psub = tid & 7;
    const int prow8 = BROW(row0 + prl);
    f32x4 ph[3], php[4];
    float pac[4];
    if (net == IQLHIP_NET_PI) {
      const float* hsb = q_heads;
      const unsigned oh = (unsigned)prow8 * (unsigned)HEAD_LD;
      ph[0] = *(const f32x4*)(hsb + (oh + 4u)); ph[1] = *(const f32x4*)(hsb + (oh + 8u)); ph[2] = *(const f32x4*)(hsb + (oh + 12u));
      const float* arow = q_xb + (unsigned)(prow8 * h_ld + h_S);
      const f32x4* hp = (const f32x4*)(q_heads + MB * HEAD_LD + (unsigned)(prow8 * h_A * NSPLIT));
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        php[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
        pac[c] = 0.f;
        if (c == 0 || 8 * c < h_A) {               // block-uniform: dims >= 8 only for wide action spaces
          const int dd = min(psub + 8 * c, h_A - 1);
          php[c] = hp[dd];
          pac[c] = arow[dd];
        }
      }
    }
    // W2 rows matching this thread's H1 columns (all threads use cols 4*(tid&63)): row 0 for the scalar
    // heads, rows 0..7 for the policy (issued now, ahead of the W1 stream; rows >= 8 are loaded later)
    const int j4 = tid & 63;
    const f32x4 w2v = *(const f32x4*)(w2 + 4 * j4);
    f32x4 w2v8[8];
    if (D > 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) w2v8[j] = *(const f32x4*)(w2 + min(j, D - 1) * HID + 4 * j4);
    }
    // H1 tile [32][256] as float4 f = tid + 256q: row f>>6, cols 4*(f&63)
    // (the first half of the tile here, the second half and the H0 mask BEHIND the loss arithmetic below: the wave is busy
    //  issuing loads for ~2 k cycles — the CU's one vector-memory pipe — while the per-row inputs requested first are back
    //  after half of that; the policy's (row, dim) terms then run inside the issue phase, cf. the dW1 blocks)
    typename Frag4<BF16>::type h1v[8];
#define H1V_LOAD(q0_, q1_)                                                                              \
    _Pragma("unroll") for (int q = (q0_); q < (q1_); ++q) {                                             \
      const int f = tid + 256 * q;                                                                      \
      const unsigned row = (unsigned)BROW(row0 + (f >> 6));   /* rows >= B: dY = 0 -> dH1 = 0 */        \
      h1v[q] = ld4<BF16>(H1g, row * (unsigned)HID + (unsigned)(4 * (f & 63)));                          \
    }
    H1V_LOAD(0, 4);
    // W1 fragments: k = j in [64*wave, +64), n = i0 + 4*l15 + t — requested after the dY barrier (below): 16 KiB
    // per wave of fragment-shaped loads take ~1.5 k cycles of the CU's vector-memory pipe to issue, which in front of
    // the loss arithmetic only delayed it; issued there they stream in under the dH1 tile phase
    // FULLB (bf16, large batches): the waves split the COLUMNS (64 each) instead of the k range — no cross-wave
    // reduction — and walk all 256 k in 8 blocks of 32; ALL 64 fragments of the wave (128 registers) are requested during
    // the dH1 tile phase: fetched two k-blocks ahead the product waited ~1 k cycles per k-block for them
    constexpr bool FULLB = BF16 && MULTI;
    typename Frag4<BF16>::type bw[FULLB ? 64 : 16];      // (bf16 path: np.w1 addresses the bf16 shadow of W1)
    // H0 mask slice [32][64] as float4 f = tid + 256q: row f>>4, cols i0 + 4*(f&15)
    typename Frag4<BF16>::type h0v[2];
    const int n_x = RT_ROWS * ld / 4;
    const int x_last = B * ld / 4 - 1;
    PIN_REST();
    const float dscale = (net == IQLHIP_NET_PI && p.drop_bits != nullptr) ? p.drop_scale : 1.f;

    const PiConst pc = pi_consts_hot(p, h_pol, net, lsr);
    if (net == IQLHIP_NET_PI) {
      const float tq = fminf(sum4(ph[1]), sum4(ph[2]));
      const float u = tq - sum4(ph[0]);
      float w = fminf(expf(p.hy.beta * u), p.hy.exp_adv_max);
      if constexpr (RW) w *= rwc;
      const bool rvalid = (row0 + prl) < B;
      const bool gauss = (h_pol == IQLHIP_POLICY_GAUSSIAN);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int dd = psub + 8 * c;
        if (dd < Dp) {
          float dy = 0.f;
          const int ddc = min(dd, h_A - 1);
          const float ivar = __shfl(pc.ivar, ddc);        // lane ddc holds dim ddc's constants; whole wave active
          if (rvalid && dd < h_A) {
            const float mu = tanh_via_exp(sum4(php[c]));
            const float diff = pac[c] - mu;
            const float dmu = gauss ? (-(w * diff) * ivar) * p.inv_batch : (-2.f * w * diff) * p.inv_batch;
            dy = dmu * (1.f - mu * mu);
          }
          dYs[prl * DYLD + dd] = dy;
        }
      }
    } else if (tid < RT_ROWS) {
      const int row = row0 + tid;
      float la, lbv;
      float* dyrow = dYs + tid * DYLD;
      for (int dd = 0; dd < Dp; ++dd) dyrow[dd] = 0.f;
      if (row < B) {
        row_finish(p, net, in, dyrow, la, lbv);
        if constexpr (RW) dyrow[0] *= rwc;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    H1V_LOAD(4, 8);
#undef H1V_LOAD
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = tid + 256 * q;
      const unsigned row = (unsigned)BROW(row0 + (f >> 4));
      h0v[q] = ld4<BF16>(H0g, row * (unsigned)HID + (unsigned)(i0 + 4 * (f & 15)));
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    STAMP(p, 5);
    // (requested two at a time between the row groups of the dH1 tile below: the four waves' 64 KB take ~1 k cycles of
    //  the CU's 64 B/clk fill path, which the tile's arithmetic covers instead of waiting behind it)
    // W1 row (= k index j of dH0 = dH1 . W1) of fragment ks: fp32 k = 4 ks + g (+ 64 wave); bf16: the bf16 MFMA's native map,
    // 8 CONTIGUOUS k per lane group — k = 32 (ks >> 3) + 8 g + (ks & 7) — so that the dH1 operand is ONE 16-byte LDS read.
    // FULLB: fragment ks = 8 kb + e of k-block kb: row 32 kb + 8 g + e, columns 64 wave + 4 l15 ..
#define BWB_ROW(ks_) (FULLB ? (32 * ((ks_) >> 3) + 8 * g + ((ks_) & 7)) : (BF16 ? (64 * wave + 32 * ((ks_) >> 3) + 8 * g + ((ks_) & 7)) : (64 * wave + 4 * (ks_) + g)))
#define BWB_COL (FULLB ? (64 * wave + 4 * l15) : (i0 + 4 * l15))
#define BWB_LOAD(ks_) bw[ks_] = ld4<BF16>(w1, (unsigned)(BWB_ROW(ks_) * HID + BWB_COL))

    // dH1s[r][j] = (sum_dd dY[r][dd] W2[dd][j]) * (H1[r][j] > 0)
    if (D > 8) {
      // wide heads (policy with more than 8 action dims): 8 dims at a time, the chunk's 8 W2 rows loaded ONCE (the
      // next chunk's while this one is multiplied) and used for all 8 rows of the thread; dY rows are zero-filled
      // to Dp, so rows >= D of a chunk (clamped duplicates) add exact zeros — same sums, same order as per-row code
      f32x4 sacc[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) sacc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
      f32x4 wv[8], wn[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) wv[j] = w2v8[j];
      for (int d0 = 0; d0 < D; d0 += 8) {
        const bool more = (d0 + 8 < D);
        if (more) {
#pragma unroll
          for (int j = 0; j < 8; ++j) wn[j] = *(const f32x4*)(w2 + min(d0 + 8 + j, D - 1) * HID + 4 * j4);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int rl = (tid + 256 * q) >> 6;
          const f32x4 ya = *(const f32x4*)(dYs + rl * DYLD + d0), yb = *(const f32x4*)(dYs + rl * DYLD + d0 + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) sacc[q] += ya[j] * wv[j];
#pragma unroll
          for (int j = 0; j < 4; ++j) sacc[q] += yb[j] * wv[4 + j];
        }
        if (more) {
#pragma unroll
          for (int j = 0; j < 8; ++j) wv[j] = wn[j];
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int rl = (tid + 256 * q) >> 6;
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = ((float)h1v[q][e] > 0.f) ? sacc[q][e] * dscale : 0.f;
        if constexpr (BF16) {
          bf16x4 ob_;
#pragma unroll
          for (int e = 0; e < 4; ++e) ob_[e] = (__bf16)out[e];
          *(bf16x4*)(dH1b + rl * H0B_LD + 4 * j4) = ob_;
        } else {
          *(f32x4*)(dH1s + rl * H0_LD + 4 * j4) = out;
        }
        if constexpr (FULLB) {
#pragma unroll
          for (int e = 0; e < 8; ++e) BWB_LOAD(8 * q + e);
        } else {
          BWB_LOAD(2 * q);
          BWB_LOAD(2 * q + 1);
        }
      }
    } else {
      // (the dY reads of the whole tile in one batch per net kind, then the arithmetic: with the kind's branch inside the row
      //  loop every row group was an LDS round trip of its own — read, wait, multiply, write)
      f32x4 sq[8];
      if (D == 1) {
        float dy1[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) dy1[q] = dYs[((tid + 256 * q) >> 6) * DYLD];
#pragma unroll
        for (int q = 0; q < 8; ++q) sq[q] = dy1[q] * w2v;
      } else {
        // dYs is zero-filled up to Dp >= 8 and w2v8[j >= D] repeats row D-1: unconditional float4 LDS reads, four row groups
        // at a time (registers)
#pragma unroll
        for (int hq = 0; hq < 2; ++hq) {
          f32x4 ya[4], yb[4];
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int rl = (tid + 256 * (4 * hq + qq)) >> 6;
            ya[qq] = *(const f32x4*)(dYs + rl * DYLD);
            yb[qq] = *(const f32x4*)(dYs + rl * DYLD + 4);
          }
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            f32x4 s = ya[qq][0] * w2v8[0];
#pragma unroll
            for (int j = 1; j < 4; ++j) s += ya[qq][j] * w2v8[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) s += yb[qq][j] * w2v8[4 + j];
            sq[4 * hq + qq] = s;
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int rl = (tid + 256 * q) >> 6;
        const f32x4 s = sq[q];
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = ((float)h1v[q][e] > 0.f) ? s[e] * dscale : 0.f;
        if constexpr (BF16) {
          bf16x4 ob_;
#pragma unroll
          for (int e = 0; e < 4; ++e) ob_[e] = (__bf16)out[e];
          *(bf16x4*)(dH1b + rl * H0B_LD + 4 * j4) = ob_;
        } else {
          *(f32x4*)(dH1s + rl * H0_LD + 4 * j4) = out;
        }
        if constexpr (FULLB) {
#pragma unroll
          for (int e = 0; e < 8; ++e) BWB_LOAD(8 * q + e);
        } else {
          BWB_LOAD(2 * q);
          BWB_LOAD(2 * q + 1);
        }
      }
    }
    __syncthreads();
    STAMP(p, 6);
    if constexpr (FULLB) {
      // ===== bf16, large batches: the whole row tile in one pass (host: 4 slices per (b) block, i0 = 0).  Per slice
      // the old structure paid three barriers, a cross-wave reduction through LDS and a dozen dependent LDS round
      // trips for ~300 cycles of matrix work (8 k cycles per slice at 1 024 rows, profiles/r03_stamps_config5_1024_bf16.txt).
      // Here wave w owns columns [64 w, 64 w + 64) of dH0 = dH1 . W1 over ALL 256 k (8 k-blocks of 32, the W1 shadow's
      // fragments double-buffered in registers), masks them in registers, parks them TRANSPOSED (bf16 [col][row]) for the
      // dW0 product — whose operands then are one 16-byte LDS read each — and stores its 64 rows of [dW0 | db0].
      typename Frag4<true>::type hm[2][4];          // H0 mask in accumulator layout: rows 16 rt + 4 g + reg, cols 64 w + 4 l15 ..
#pragma unroll
      for (int rtl = 0; rtl < 2; ++rtl)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const unsigned row = (unsigned)BROW(row0 + 16 * rtl + 4 * g + reg);
          hm[rtl][reg] = ld4<true>(H0g, row * (unsigned)HID + (unsigned)(64 * wave + 4 * l15));
        }
      f32x4 xr[XR_MAX_F4];
      xr_load(xr, q_xb, row0 * ld / 4, n_x, x_last);
      bf16x8 Ad[2][8];
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) {
        Ad[0][kb] = *(const bf16x8*)(dH1b + l15 * H0B_LD + 32 * kb + 8 * g);
        Ad[1][kb] = *(const bf16x8*)(dH1b + (16 + l15) * H0B_LD + 32 * kb + 8 * g);
      }
      f32x4 acc[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) {
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) {
          bf16x8 Bv;
#pragma unroll
          for (int e = 0; e < 8; ++e) Bv[e] = bw[8 * kb + e][tb];
          acc[0][tb] = MFMA_BF16(Ad[0][kb], Bv, acc[0][tb]);
          acc[1][tb] = MFMA_BF16(Ad[1][kb], Bv, acc[1][tb]);
        }
      }
      STAMP(p, 7);
      constexpr int TLD = 40;                         // row stride of the transposed tile: 80 bytes, conflict-free 16-byte reads
      __bf16* dH0T = (__bf16*)red;                    // [256][TLD]
#pragma unroll
      for (int rtl = 0; rtl < 2; ++rtl)
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) {
          bf16x4 o;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            o[reg] = (__bf16)(((float)hm[rtl][reg][tb] > 0.f) ? acc[rtl][tb][reg] * dscale : 0.f);    // rows >= B carry 0
          *(bf16x4*)(dH0T + (64 * wave + 4 * l15 + tb) * TLD + 16 * rtl + 4 * g) = o;
        }
      xr_store(xr, Xr, n_x);
      __syncthreads();
      STAMP(p, 8);
      // [dW0 | db0][i][kc] = sum_r dH0[r][i] [X | 1][r][kc]: A = [X | 1] (m = kc, k = row 8 g + e), B = dH0T (n = i, k = row)
      const int k1 = k0 + 1;
      const int nct = (k1 + 15) >> 4;
      bf16x8 Ax[9];
#pragma unroll
      for (int ct = 0; ct < 9; ++ct) {
        if (ct < nct) {
          const int kc = 16 * ct + l15;
          const int kcc = min(kc, k0 - 1);
          float a8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xa = Xr[(8 * g + e) * ld + xoff + kcc];
            a8[e] = (kc < k0) ? xa : ((kc == k0) ? 1.f : 0.f);      // ones column -> db0
          }
          Ax[ct] = pack8s(a8);
        }
      }
      float* slabB = p.sc.slab_b + p.sc.slab_b_off[net] + rt * (HID * k0 + HID);
      float* dstB = slabB + HID * k0;
      STAMP(p, 12);
#pragma unroll
      for (int itl = 0; itl < 4; ++itl) {
        const int il = 64 * wave + 16 * itl + l15;
        const bf16x8 Bd = *(const bf16x8*)(dH0T + il * TLD + 8 * g);
#pragma unroll
        for (int ct = 0; ct < 9; ++ct) {
          if (ct < nct) {
            const f32x4 r4 = MFMA_BF16(Ax[ct], Bd, ((f32x4){0.f, 0.f, 0.f, 0.f}));
            const int kc0 = 16 * ct + 4 * g;
            if (kc0 + 3 < k0) {
              *(f32x4u*)(slabB + (unsigned)(il * k0 + kc0)) = r4;
            } else {
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) {
                const int kc = kc0 + reg;
                if (kc < k0) slabB[(unsigned)(il * k0 + kc)] = r4[reg];
                else if (kc == k0) dstB[il] = r4[reg];
              }
            }
          }
        }
      }
      STAMP(p, 9);
      RT_STAMP(p, 14, rt_entry_);
      RT_STAMP(p, 15, iql_realtime());
      return;
    }
    // the 32 packed rows, needed last (dW0): issued only now — the H1 / W2 registers are free again, the loads
    // queue behind the W1 fragments (so waiting for those does not wait for these) and the MFMA phase hides them
    f32x4 xr[XR_MAX_F4];
    xr_load(xr, q_xb, row0 * ld / 4, n_x, x_last);

    // ======== per column slice (one pass unless MULTI): dH0 slice, dW0 / db0 slice.  The next slice's W1 fragments are
    // requested into the registers this slice's MFMAs have just consumed, its H0 mask under the MFMA phase.
    for (int itn = 0;; ++itn) {
    const bool more = MULTI && (itn + 1 < (1 << bsl2));
    typename Frag4<BF16>::type h0n[2] = {h0v[0], h0v[1]};

    // dH0 partial over this wave's 64 j's: [32 rows][64 cols]
    {
      f32x4 acc[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (BF16) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {     // k = j index: 64w + 32q + 8g + e, e = 0..7 — one 16-byte read per operand
          const bf16x8 A0 = *(const bf16x8*)(dH1b + l15 * H0B_LD + 64 * wave + 32 * q + 8 * g);
          const bf16x8 A1 = *(const bf16x8*)(dH1b + (16 + l15) * H0B_LD + 64 * wave + 32 * q + 8 * g);
#pragma unroll
          for (int tb = 0; tb < 4; ++tb) {
            bf16x8 Bv;                        // (the W1 shadow arrives as bf16: assembled, not converted)
#pragma unroll
            for (int e = 0; e < 8; ++e) Bv[e] = bw[8 * q + e][tb];
            acc[0][tb] = MFMA_BF16(A0, Bv, acc[0][tb]);
            acc[1][tb] = MFMA_BF16(A1, Bv, acc[1][tb]);
          }
          if (more) {
#pragma unroll
            for (int ks = 8 * q; ks < 8 * q + 8; ++ks)
              bw[ks] = ld4<BF16>(w1, (unsigned)(BWB_ROW(ks) * HID + i0 + 64 + 4 * l15));
          }
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          const int kk = 64 * wave + 4 * ks + g;
          const float a0 = dH1s[l15 * H0_LD + kk];
          const float a1 = dH1s[(16 + l15) * H0_LD + kk];
#pragma unroll
          for (int tb = 0; tb < 4; ++tb) {
            acc[0][tb] = MFMA16(a0, bw[ks][tb], acc[0][tb]);
            acc[1][tb] = MFMA16(a1, bw[ks][tb], acc[1][tb]);
          }
          if ((ks & 3) == 3 && more) {
#pragma unroll
            for (int k2 = ks - 3; k2 <= ks; ++k2)
              bw[k2] = ld4<BF16>(w1, (unsigned)((64 * wave + 4 * k2 + g) * HID + i0 + 64 + 4 * l15));
          }
        }
      }
      if (more) {      // the next slice's H0 mask
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int f = tid + 256 * q;
          const unsigned row = (unsigned)BROW(row0 + (f >> 4));
          h0n[q] = ld4<BF16>(H0g, row * (unsigned)HID + (unsigned)(i0 + 64 + 4 * (f & 15)));
        }
      }
      float* myred = red + wave * 32 * T64_LD;
#pragma unroll
      for (int rtile = 0; rtile < 2; ++rtile)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int rl = 16 * rtile + 4 * g + reg;
          f32x4 v = (f32x4){acc[rtile][0][reg], acc[rtile][1][reg], acc[rtile][2][reg], acc[rtile][3][reg]};
          *(f32x4*)(myred + rl * T64_LD + 4 * l15) = v;
        }
    }
    // park the packed rows for the dW0 product
    if (itn == 0) xr_store(xr, Xr, n_x);
    __syncthreads();
    STAMP(p, 7);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = tid + 256 * q;
      const int rl = f >> 4, i4 = f & 15;
      f32x4 s = *(const f32x4*)(red + rl * T64_LD + 4 * i4);
#pragma unroll
      for (int w = 1; w < 4; ++w) s += *(const f32x4*)(red + w * 32 * T64_LD + rl * T64_LD + 4 * i4);
      f32x4 out;
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = ((float)h0v[q][e] > 0.f) ? s[e] * dscale : 0.f;   // rows >= B carry s = 0
      *(f32x4*)(dH0s + rl * T64_LD + 4 * i4) = out;
    }
    __syncthreads();

    STAMP(p, 8);
    float* slabB = p.sc.slab_b + p.sc.slab_b_off[net] + rt * (HID * k0 + HID);
    // [dW0 | db0][i][kc] partial = sum_r dH0[r][i] * [X | 1][r][kc].  A = [X|1] (m = kc), B = dH0 (n = i):
    // a lane's 4 accumulator registers are 4 consecutive kc of one i.  This wave: i in [i0 + 16*wave, +16).
    {
      // (multi-slice blocks: this block's lane masks — kc < k0, kc == k0, kc0 + 3 < k0 per column tile and register — are
      //  loop-invariant; hipcc hoisted all ~80 of them, as 64-bit masks, in front of the slice loop and spilled 170-180
      //  SGPRs to keep them alive across it.  A per-iteration copy of k0 the compiler cannot see through keeps them where
      //  they are used.  The outer name is shadowed on purpose.)
      int k0_ = k0;
      if constexpr (MULTI) asm volatile("" : "+s"(k0_));
      const int k0 = k0_;
      const int k1 = k0 + 1;
      const int nct = (k1 + 15) >> 4;
      f32x4 acc[9];
#pragma unroll
      for (int ct = 0; ct < 9; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
      float bv[8];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) bv[ks] = dH0s[(4 * ks + g) * T64_LD + 16 * wave + l15];
#pragma unroll
      for (int ct = 0; ct < 9; ++ct) {
        if (ct < nct) {
          const int kc = 16 * ct + l15;
          const int kcc = min(kc, k0 - 1);
          float xa[8];
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) xa[ks] = Xr[(4 * ks + g) * ld + xoff + kcc];
          if (BF16) {      // the tile's 32 rows are ONE bf16 MFMA (lane group g holds rows 4 ks + g of both operands)
            float a8[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) a8[ks] = (kc < k0) ? xa[ks] : ((kc == k0) ? 1.f : 0.f);
            acc[ct] = MFMA_BF16(pack8s(a8), pack8s(bv), acc[ct]);
          } else {
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
              const float a = (kc < k0) ? xa[ks] : ((kc == k0) ? 1.f : 0.f);   // ones column -> db0
              acc[ct] = MFMA16(a, bv[ks], acc[ct]);
            }
          }
        }
      }
      STAMP(p, 12);
      // straight from the accumulators into the row-tile slab: a lane's 4 registers of a tile are 4 consecutive kc of one
      // i, i.e. 16 contiguous bytes of the [i][kc] slab (4-byte aligned: k0 is odd as often as not) — one unaligned
      // 16-byte store where the whole run lies below k0, single words around the k0 column (= db0).  Staging the tile in
      // LDS for aligned float4 stores cost a barrier and two passes (1.8 k cycles of every (b) block's tail).
      {
        float* dstW = slabB + i0 * k0;
        float* dstB = slabB + HID * k0 + i0;
        const int il = 16 * wave + l15;
#pragma unroll
        for (int ct = 0; ct < 9; ++ct) {
          if (ct < nct) {
            const int kc0 = 16 * ct + 4 * g;
            if (kc0 + 3 < k0) {
              *(f32x4u*)(dstW + (unsigned)(il * k0 + kc0)) = acc[ct];
            } else {
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) {
                const int kc = kc0 + reg;
                if (kc < k0) dstW[(unsigned)(il * k0 + kc)] = acc[ct][reg];
                else if (kc == k0) dstB[il] = acc[ct][reg];
              }
            }
          }
        }
      }
    }
    if (!more) break;
    h0v[0] = h0n[0]; h0v[1] = h0n[1];
    i0 += 64;
    }   // (red / dH0s of the next slice are written behind its own barriers: every thread has left this slice's dW0 reads)
    STAMP(p, 9);
    RT_STAMP(p, 14, rt_entry_);
    RT_STAMP(p, 15, iql_realtime());
  }

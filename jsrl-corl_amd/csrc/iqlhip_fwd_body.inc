// Body of the forward — included by iql_fwd_kernel and iql_fwd_group_kernel (iqlhip_kernels.h):
// ONE body for the single-agent kernel and its trainer-group form, so the arithmetic exists once.  blockIdx.x / gridDim.x
// are the block's index and grid size of ONE agent's launch in both (a group kernel's agent is blockIdx.y).
// In scope: template flags BF16, W0DMA, MULTI, ONE, MIXED_IDLE (the idle blocks' work is a two-source chunk's; 2: a weighted chunk's), the
// agent's `p` (StepParams) and ROW_EXIT: a block whose row tile
// lies outside the agent's batch exits under every block map (iql_fwd_group_kernel only: its grid.x is the largest
// member's; a single agent's one- and two-slice grids are sized exactly and compile without the test).
// EARLY (iql_fwd_kernel_early only; everywhere else false, and the leading arguments q_* null constants: FWD_NOT_EARLY()):
// the one-slice fp32 forward whose every instance stages W0 in LDS through registers (k0 <= 32, packed rows of at most
// 3 float4 per thread).  Every address of the issue section is formed from the PRELOADED leading arguments q_*, so the
// small operands leave before the by-value `p` has arrived, and the first FWD_EARLY_W1 of the wave's 16 W1 fragment loads
// follow them at once, in front of the LDS stores and the barrier (the wait there is a counted one that leaves them in
// flight); layer 0's MFMA loop hosts the other 12.  Same loads, same k-maps, same arithmetic as the other
// instantiations, which `if constexpr` keeps instruction for instruction as they were.
  RT_ENTRY();
  const int bid = blockIdx.x;
  // XCD-affine block map (consecutive workgroups go round the 8 XCDs: XCD x = blockIdx & 7).  Across a kernel boundary an
  // XCD reads back what it wrote ITSELF much faster than what another XCD wrote (profiles/r01_l2_retention_microbench.txt:
  // 11.7 vs 20.4 us for the same reads; the L2's FETCH_SIZE counters are the same either way — r03_pmc_summary.json — so
  // the difference is on the memory side of the L2).  So the three kernels agree on who touches what: XCDs n and n + 4 belong to net
  // n (V, Q1, Q2, pi) — the backward's blocks of net n run there, the update kernel's blocks there own the net's arena
  // segment in 64-float stripes (even stripes on XCD n, odd ones on n + 4; W1 [unit][k] leads the segment with 4 stripes
  // per row, so the k-slice i of W1 — a dW1 tile's columns, a (b) block's slice — is the stripes of parity i & 1), and
  // HERE the two forward instances that read net n's
  // weights (or their target copy) share those two XCDs by column slice: slices of parity h on XCD n + 4 h.
  //   XCD pair   0 / 4          1 / 5       2 / 6       3 / 7
  //   instances  V(s), V(s')    Q1, Qt1     Q2, Qt2     pi, idle            (which = bit 0 of the block's index on its XCD)
  // One-slice grids: the H0 columns a block saves are the ones the backward's dW1 tiles and (b) slices of the same parity
  // read on this XCD (its own W1 rows span all k: half of their stripes were written here, half on the partner XCD —
  // for every block alike, whatever the map).  Blocks that walk 2 slices take the
  // pair {2 h, 2 h + 1}; blocks that walk all 4 take the row tiles of parity h.
  const int fx = bid & 7, fh = fx >> 2, fr = bid >> 3;
  constexpr unsigned FWD_PAIR_A = 0x6541u, FWD_PAIR_B = 0x7320u;      // nibble (x & 3): V(s) Q1 Q2 pi | V(s') Qt1 Qt2 idle
  const int inst = ONE ? p.only_inst : (int)((((fr & 1) ? FWD_PAIR_B : FWD_PAIR_A) >> (4 * (fx & 3))) & 7u);
  if (inst >= 7) {     // the idle eighth of the grid: the chunk's bookkeeping for the NEXT step (graph chunks), else exits
    if (p.g_work) idle_block_work<MIXED_IDLE>(p.g_work, (fr >> 1) * 2 + fh, (int)(gridDim.x >> 3));
    return;
  }
  const int spb_l2 = MULTI ? (p.spb_l2 & 3) : 0;      // (MULTI = false: exactly the one-slice code, no loop)
  const int spb = 1 << spb_l2;
  int ns, rt;
  if (ONE) {           // blockIdx = row tile * NSPLIT + column slice
    ns = bid & (NSPLIT - 1);
    rt = bid >> 2;
  } else if (spb_l2 == 0) {
    ns = 2 * ((fr >> 1) & 1) + fh;
    rt = fr >> 2;
    if (ROW_EXIT && rt * RT_ROWS >= p.rows) return;
  } else if (spb_l2 == 1) {
    ns = 2 * fh;
    rt = fr >> 1;
    if (ROW_EXIT && rt * RT_ROWS >= p.rows) return;
  } else {
    ns = 0;
    rt = 2 * (fr >> 1) + fh;
    if (rt * RT_ROWS >= p.rows) return;      // (odd row-tile counts: the grid is rounded up to pairs of row tiles)
  }
  const int row0 = rt * RT_ROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;

  // EARLY: the instance's tensors from the preloaded arena pointers and dims (instances V(s'), V(s), Qt1, Qt2, Q1, Q2, pi;
  // the target instances read the target arena, whose pointer is biased so that the parameter arena's offsets hold in
  // it; W1 leads a net's segment).  xoff, slot and the activation / head pointers are not needed to issue a load: they
  // come from `p` behind the issue section (below, behind the W1 loads).
  const int e_net = (inst < 2) ? IQLHIP_NET_V : ((inst == 6) ? IQLHIP_NET_PI : IQLHIP_NET_Q1 + (inst & 1));
  const ArenaOff e_ao = arena_off(EARLY ? e_net : 0, (int)(q_dims & 255u), (int)((q_dims >> 8) & 63u),
                                  (int)((q_dims >> 14) & 1u) == IQLHIP_POLICY_GAUSSIAN);
  const float* const e_base = (inst == 2 || inst == 3) ? q_target : q_params;
  const NetPtrs np = EARLY ? NetPtrs{e_base + e_ao.w0, e_base + e_ao.b0, e_base + (e_ao.w0 - 65536u), e_base + e_ao.b1,
                                     e_base + e_ao.w2, e_base + e_ao.b2, e_ao.k0, e_ao.d}
                           : p.inst[inst];
  int xoff = EARLY ? 0 : p.xoff[inst];
  int slot = EARLY ? -1 : p.slot[inst];
  const int k0 = np.k0;
  const int k0p = (k0 + 3) & ~3;
  const int D = np.d;
  const int ld = EARLY ? (int)(q_ldB & 1023u) : p.ld;
  const int B = EARLY ? (int)(q_ldB >> 10) : p.rows;
  const int w0k = EARLY ? FWD_EARLY_MAX_K : p.w0_lds_k;   // (EARLY: the host launches it only when every k0 is at most this, and staged)
  const float* xb = EARLY ? q_xb : p.xb;
  float* h0g = EARLY ? nullptr : p.sc.h0;
  float* h1g = EARLY ? nullptr : p.sc.h1;
  float* headsg = EARLY ? nullptr : p.sc.heads;
  const int MB = EARLY ? (int)q_mb : p.sc.max_batch;
  const int Aact = EARLY ? (int)((q_dims >> 8) & 63u) : p.A;
  if constexpr (!EARLY) {
    PIN_P(np.w0); PIN_P(np.b0); PIN_P(np.w1); PIN_P(np.b1); PIN_P(np.w2); PIN_P(np.b2);
    PIN_S(k0); PIN_S(D); PIN_S(xoff); PIN_S(slot); PIN_S(ld); PIN_S(B); PIN_S(MB); PIN_S(Aact);
    PIN_P(xb); PIN_P(h0g); PIN_P(h1g); PIN_P(headsg); PIN_S(w0k);
  }
  const bool w0_lds = EARLY ? true : (W0DMA ? (k0 <= w0k) : (k0 <= min(w0k, W0_LDS_MAX_K)));
  const bool w0_dma = W0DMA && w0_lds && (k0 > W0_LDS_MAX_K);      // wide inputs: copied by LDS-DMA, no staging registers

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* H0s = smem;                         // [32][H0_LD]
  float* H1s = H0s + RT_ROWS * H0_LD;        // [32][T64_LD]
  float* Xr = H1s + RT_ROWS * T64_LD;        // [32][ld]  packed rows of this tile
  // (regions sized by the ACTUAL dims, not the limits: at S=17/A=6 the block needs 75 KB instead of 109 KB, so two
  //  blocks fit a CU's 160 KB when a large batch brings more than one block per CU; host: fwd_lds_floats())
  // [Dp][W2_LD] head weights of this column slice (rows beyond D zero: MFMA operand), then b2[D]; D <= A
  float* W2s = Xr + RT_ROWS * ld;
  const int w2s_words = ((Aact + 15) & ~15) * W2_LD + 32;
  unsigned* Mk = (unsigned*)(W2s + w2s_words);       // [2][32][8] dropout keep-bits of the tile
  float* W0s = W2s + w2s_words + 512;        // [256*k0] flat copy of layer-0 weights (when w0_lds); 16-B aligned
  // (no integer casts on LDS pointers: they would demote every access to a flat load, and a flat load
  //  waits vmcnt(0) — it would drain the W1 stream that is meant to stay in flight under layer 0)

  STAMP_BASE(p, 0);
  STAMP(p, 0);
  // ======== issue every global load of the block.  vmcnt retires in issue order: the small operands of
  // layer 0 go first, the 64 KiB W1 slice last — it keeps streaming while layer 0 runs (no LDS-DMA
  // here: a DMA in flight would make __syncthreads() wait vmcnt(0), i.e. for W1 as well).
  // (a) the 32 packed input rows, contiguous in xb: n_x float4, clamped at the end of the batch
  const int n_x = RT_ROWS * ld / 4;
  const int x_last = B * ld / 4 - 1;
  f32x4 xr[XR_MAX_F4];
  if constexpr (EARLY) {      // (n_x <= 3 * 256 on this path: no run-time trip count between the loads)
#pragma unroll
    for (int q = 0; q < XR_MAX_F4; ++q) xr[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    xr_issue<0, 3>(xr, xb, row0 * ld / 4, n_x, x_last);
  } else {
    xr_load(xr, xb, row0 * ld / 4, n_x, x_last);
  }
  // (b) head weights of this slice + b2, biases
  f32x4 w2pre[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = min(tid + 256 * q, D * 16 - 1);
    w2pre[q] = *(const f32x4*)(np.w2 + (unsigned)((e >> 4) * HID + ns * 64 + 4 * (e & 15)));
  }
  const float b2v = np.b2[min(tid, D - 1)];
  f32x4 bias0[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) bias0[ct] = *(const f32x4*)(np.b0 + (unsigned)(wave * 64 + ct * 16 + 4 * g));
  f32x4 bias1 = *(const f32x4*)(np.b1 + (unsigned)(ns * 64 + wave * 16 + 4 * g));
  // (b2) dropout keep-bits of this row tile (policy instance only): thread -> (row tid >> 3, word tid & 7)
  const bool drop = (inst == 6) && ((EARLY ? q_drop : p.drop_bits) != nullptr);
  unsigned mk0 = 0xFFFFFFFFu, mk1 = 0xFFFFFFFFu;
  if constexpr (EARLY) {
    // unconditional (a load inside a branch makes the join wait vmcnt(0), and W1 is to stay in flight across it):
    // blocks without dropout read the first words of the batch instead and discard them
    const int mrow = min(row0 + (tid >> 3), B - 1);
    const unsigned* const dsrc = drop ? q_drop : (const unsigned*)q_xb;
    const unsigned l0w = *(dsrc + (unsigned)(drop ? mrow * 8 + (tid & 7) : 0));
    const unsigned l1w = *(dsrc + (unsigned)(drop ? (MB + mrow) * 8 + (tid & 7) : 0));
    mk0 = l0w;      // (raw until the LDS store below)
    mk1 = l1w;
  } else if (drop) {
    const int mrow = min(row0 + (tid >> 3), B - 1);
    mk0 = p.drop_bits[mrow * 8 + (tid & 7)];
    mk1 = p.drop_bits[(MB + mrow) * 8 + (tid & 7)];
  }
  // (c) layer-0 weights: flat float4 copy of 64*k0 float4 (thread handles tid + 256 j); 8 loads cover k0 <= 32
  const int n_w0v = 64 * k0;
  f32x4 w0v[16];
  if (w0_dma) {
    // whole waves of 64 x 16 B: global (per-lane address, clamped) -> LDS (wave base + lane * 16); the tail wave
    // writes into the region's 4 KiB slack.  The barrier below then waits for every outstanding load (the DMA is
    // tracked by vmcnt), so on this path the W1 fragments are requested after it and stream in under layer 0.
    const int nj = (n_w0v + 255) >> 8;
    for (int j = 0; j < nj; ++j)
      lds_dma16(np.w0 + 4 * min(tid + 256 * j, n_w0v - 1), W0s + 4 * (256 * j + 64 * wave));
  } else if (w0_lds) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w0v[j] = *(const f32x4*)(np.w0 + 4u * (unsigned)min(tid + 256 * j, n_w0v - 1));
    if (!EARLY && k0 > 32) {
#pragma unroll
      for (int j = 8; j < 16; ++j) w0v[j] = *(const f32x4*)(np.w0 + 4u * (unsigned)min(tid + 256 * j, n_w0v - 1));
    }
  }
  // (d) this wave's W1 rows (16 output units x 256 k) as MFMA fragments: 64 KiB per block
  int n1 = ns * 64 + wave * 16 + l15;  // hidden-1 unit of this lane
  // fp32: 16 fragments of 4 k (k = 16 ks + 4 g + t).  bf16 (np.w1 addresses the bf16 shadow of W1): 8 fragments of 8
  // CONTIGUOUS k (k = 32 j + 8 g + e) — the bf16 MFMA's native operand, one 16-byte load each; the H0 tile in LDS is
  // bf16 too and is read with the same map, one ds_read_b128 per operand, no conversion anywhere in layer 1.
  f32x4 bw[BF16 ? 1 : 16];
  bf16x8 bwb[BF16 ? 8 : 1];
  __bf16* H0b = (__bf16*)H0s;          // [32][H0B_LD] (bf16 path: the H0 tile lives here instead of H0s)
#define BW_LOAD(ks_) bw[ks_] = *(const f32x4*)(np.w1 + (unsigned)(n1 * HID + 16 * (ks_) + 4 * g))
#define BWB_AT(unit_, j_) (*(const bf16x8*)((const __bf16*)np.w1 + (unsigned)((unit_) * HID + 32 * (j_) + 8 * g)))
  if constexpr (EARLY) {
    // the first W1 fragment loads of the wave NOW, behind the small operands (vmcnt retires in issue order, and those
    // are waited for first: the wait in front of the LDS stores below is a counted one that leaves these in flight).
    // How many: a fragment load (16 lanes -> 16 rows) occupies the CU's one vector-memory pipe for ~64 cycles, so all 64
    // of a block take ~4 k cycles to issue, and a wave cannot reach its LDS stores before its last one has left.  With
    // all 16 per wave here the prologue grew from 3.1 k to 5.3 k cycles and the step LOST 0.5 us although layer 0
    // shrank by 0.85 k (profiles/fwd_early_w1_stamps_all16.txt); the small operands' round trip hides about 4 per wave
    // (2..5 measured alike, 0 and 8 worse: profiles/fwd_early_w1_ab.txt).  The fences keep hipcc from moving them
    // behind the LDS stores or mixing them into the small loads.  Then the rest of `p`, in one batch of scalar loads,
    // whose fetch has had the whole issue section to arrive.
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < FWD_EARLY_W1; ++ks) BW_LOAD(ks);
    __builtin_amdgcn_sched_barrier(0);
    xoff = p.xoff[inst];
    slot = p.slot[inst];
    h0g = p.sc.h0;
    h1g = p.sc.h1;
    headsg = p.sc.heads;
    PIN_S(xoff); PIN_S(slot); PIN_P(h0g); PIN_P(h1g); PIN_P(headsg); PIN_S(p.drop_scale);
    __builtin_amdgcn_sched_barrier(0);
  }

  xr_store(xr, Xr, n_x);
  const int Dp = (D + 15) & ~15;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = tid + 256 * q;
    if (e < Dp * 16) *(f32x4*)(W2s + (e >> 4) * W2_LD + 4 * (e & 15)) = (e < D * 16) ? w2pre[q] : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if (tid < D) W2s[Dp * W2_LD + tid] = b2v;
  if constexpr (EARLY) {
    // (the loaded words are used as loaded, here where they are waited for anyway: hipcc otherwise moves a load whose
    //  value a block discards into a branch)
    asm volatile("" : "+v"(mk0), "+v"(mk1));
    mk0 = drop ? mk0 : 0xFFFFFFFFu;
    mk1 = drop ? mk1 : 0xFFFFFFFFu;
  }
  Mk[tid] = mk0;
  Mk[256 + tid] = mk1;
  if (w0_lds && !w0_dma) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = tid + 256 * j;
      if (f < n_w0v) *(f32x4*)(W0s + 4 * f) = w0v[j];
    }
    if (!EARLY && k0 > 32) {
#pragma unroll
      for (int j = 8; j < 16; ++j) {
        const int f = tid + 256 * j;
        if (f < n_w0v) *(f32x4*)(W0s + 4 * f) = w0v[j];
      }
    }
  }
  __syncthreads();
  // the W1 fragments are requested only now: 16 x 1 KB per wave of row-fragment loads take ~1.5 k cycles of the CU's
  // one vector-memory pipe (64 B/clk) just to ISSUE — in front of the barrier they delayed layer 0 by that much.  The
  // fp32 paths with LDS-staged weights go one step further and request them BETWEEN the groups of layer-0 MFMAs (an MFMA
  // holds the SIMD's issue for 8 of its 32 cycles: four loads per 8 MFMAs trickle out at 42 B/clk over the four waves),
  // so that not even the issue time stands in front of layer 0.
  // (EARLY: they are on their way since the issue section, see there)
  const bool bw_in_l0 = !BF16 && w0_lds;
  if constexpr (BF16) {
#pragma unroll
    for (int j = 0; j < 8; ++j) bwb[j] = BWB_AT(n1, j);
  } else if (!bw_in_l0) {
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) BW_LOAD(ks);
  }
  STAMP(p, 1);

  // ---- layer 0: this wave computes H0[32][64*wave .. +64).  Operand roles: A = W0 (m = hidden unit),
  // B = X (n = row), so a lane's 4 accumulator registers are 4 consecutive hidden units of ONE row:
  // one ds_write_b128 into the row-major H0 tile.
  {
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nks = k0p >> 2;
    const float* x0 = Xr + l15 * ld + xoff;
    const float* x1 = Xr + (16 + l15) * ld + xoff;
    float bcur[4], bnxt[4], acur[2], anxt[2];
    if (w0_lds && (EARLY || nks <= 8)) {      // (EARLY: k0 <= 32, always this branch)
      // all operands of the (<= 8) k-steps are read up front, then the MFMAs run back to back
      const float* wl[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) wl[ct] = W0s + (wave * 64 + ct * 16 + l15) * k0;
      // columns kk >= k0 of a packed row hold other fields: they are zeroed on the X side (2 selects per k-step, made
      // here, in the read phase); the weight operand is read with a clamped column and used as it is (finite x 0 = 0).
      // With the selects on the four weight operands the compiler sank each v_cndmask in front of its MFMA pair
      // (VALU write -> s_nop -> MFMA, 24 times): the 48 MFMAs of this phase took 2.25 k cycles instead of 1.5 k.
      float bq[8][4], aq[8][2];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const int kk = 4 * ks + g;
        const int kc = min(kk, k0 - 1);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bq[ks][ct] = wl[ct][kc];
        const float xa = x0[kc], xb_ = x1[kc];
        aq[ks][0] = (kk < k0) ? xa : 0.f;
        aq[ks][1] = (kk < k0) ? xb_ : 0.f;
      }
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {      // (pin the selected values: no re-evaluation next to the MFMAs)
        asm volatile("" : "+v"(aq[ks][0]), "+v"(aq[ks][1]));
      }
      STAMP(p, 5);
      if constexpr (BF16) {       // (k-steps beyond nks: X side selected to zero above, weight side a clamped finite value)
        l0_chunk_bf16(acc, bq, aq);
      } else {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          if (ks < nks) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
              acc[0][ct] = MFMA16(bq[ks][ct], aq[ks][0], acc[0][ct]);
              acc[1][ct] = MFMA16(bq[ks][ct], aq[ks][1], acc[1][ct]);
            }
          }
          if (ks < 4) {       // W1 fragments 4 ks .. 4 ks + 3 behind this group of MFMAs (EARLY: those not yet requested)
#pragma unroll
            for (int k2 = 4 * ks; k2 < 4 * ks + 4; ++k2) {
              if (!EARLY || k2 >= FWD_EARLY_W1) BW_LOAD(k2);
            }
          }
        }
      }
      STAMP(p, 6);
    } else if (w0_lds) {
      // wide inputs (9..24 k-steps): chunks of 8 k-steps in straight-line code, the operands of a chunk read in one
      // batch like above and the next chunk's batch issued before this chunk's MFMAs.  (As a run-time loop with a
      // one-step look-ahead the compiler waited for each step's six reads in front of its eight MFMAs: 550 cycles
      // per k-step instead of 256.)  Only the last k-step can reach beyond k0; the selects are made per batch.
      const float* wl[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) wl[ct] = W0s + (wave * 64 + ct * 16 + l15) * k0;
      float bqA[8][4], aqA[8][2], bqB[8][4], aqB[8][2];
      auto rd = [&](float (&bq)[8][4], float (&aq)[8][2], const int base) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (base + 4 * h < nks) {
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
              const int ks = 4 * h + k4;
              const int kk = 4 * (base + ks) + g;
              const int kc = min(kk, k0 - 1);
#pragma unroll
              for (int ct = 0; ct < 4; ++ct) bq[ks][ct] = wl[ct][kc];
              const float xa = x0[kc], xb_ = x1[kc];
              aq[ks][0] = (kk < k0) ? xa : 0.f;
              aq[ks][1] = (kk < k0) ? xb_ : 0.f;
            }
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) asm volatile("" : "+v"(aq[4 * h + k4][0]), "+v"(aq[4 * h + k4][1]));
          } else if (BF16) {      // the bf16 MFMA takes all 8 k-steps of a chunk: the unread half contributes zeros
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
              aq[4 * h + k4][0] = 0.f;
              aq[4 * h + k4][1] = 0.f;
#pragma unroll
              for (int ct = 0; ct < 4; ++ct) bq[4 * h + k4][ct] = 0.f;
            }
          }
        }
      };
      auto mm = [&](const float (&bq)[8][4], const float (&aq)[8][2], const int base) {
        if constexpr (BF16) {
          l0_chunk_bf16(acc, bq, aq);
        } else {
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) {
            if (base + ks < nks) {
#pragma unroll
              for (int ct = 0; ct < 4; ++ct) {
                acc[0][ct] = MFMA16(bq[ks][ct], aq[ks][0], acc[0][ct]);
                acc[1][ct] = MFMA16(bq[ks][ct], aq[ks][1], acc[1][ct]);
              }
            }
            if (base == 0) {    // the W1 fragments, two behind each MFMA group of the first chunk
              BW_LOAD(2 * ks);
              BW_LOAD(2 * ks + 1);
            }
          }
        }
      };
      rd(bqA, aqA, 0);
      rd(bqB, aqB, 8);
      STAMP(p, 5);
      mm(bqA, aqA, 0);
      if (nks > 16) rd(bqA, aqA, 16);
      mm(bqB, aqB, 8);
      if (nks > 16) mm(bqA, aqA, 16);
      STAMP(p, 6);
    } else {
      const float* wrow[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) wrow[ct] = np.w0 + (wave * 64 + ct * 16 + l15) * k0;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) { const float v = wrow[ct][min(g, k0 - 1)]; bcur[ct] = (g < k0) ? v : 0.f; }
      for (int ks = 0; ks < nks; ++ks) {
        const int kn = 4 * (ks + 1) + g;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) { const float v = wrow[ct][min(kn, k0 - 1)]; bnxt[ct] = (kn < k0) ? v : 0.f; }
        const int kc = min(4 * ks + g, k0 - 1);
        const float a0 = x0[kc];
        const float a1 = x1[kc];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          acc[0][ct] = MFMA16(bcur[ct], a0, acc[0][ct]);
          acc[1][ct] = MFMA16(bcur[ct], a1, acc[1][ct]);
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bcur[ct] = bnxt[ct];
      }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
      for (int rtile = 0; rtile < 2; ++rtile) {
        f32x4 h;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) h[reg] = fmaxf(acc[rtile][ct][reg] + bias0[ct][reg], 0.f);
        if (drop) {   // units wave*64 + ct*16 + 4g .. +3 of row rtile*16 + l15
          const unsigned bits = Mk[(rtile * 16 + l15) * 8 + wave * 2 + (ct >> 1)] >> ((ct & 1) * 16 + 4 * g);
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) h[reg] = ((bits >> reg) & 1u) ? h[reg] * p.drop_scale : 0.f;
        }
        if constexpr (BF16) {
          bf16x4 hb_;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) hb_[reg] = (__bf16)h[reg];
          *(bf16x4*)(H0b + (rtile * 16 + l15) * H0B_LD + wave * 64 + ct * 16 + 4 * g) = hb_;
        } else {
          *(f32x4*)(H0s + (rtile * 16 + l15) * H0_LD + wave * 64 + ct * 16 + 4 * g) = h;
        }
      }
    }
  }
  STAMP(p, 7);
  __syncthreads();
  STAMP(p, 2);
#ifdef IQL_STAMPS
  // one-slice blocks (stamp 13 is the multi-slice blocks' otherwise): the cycle at which this wave's last W1 fragment
  // has landed — nothing else is in flight here, the H0 stores below not yet issued
  if constexpr (!MULTI) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(p, 13);
  }
#endif

  // ======== per column slice: layer 1 over the block's H0 tile, head partials.  One pass when the grid holds a block
  // per slice; 2 or 4 passes for large batches — the next slice's W1 fragments, head weights and bias are requested
  // right after this slice's layer-1 MFMAs and arrive under its head phase.
  for (int it = 0;; ++it) {
  const bool more = MULTI && (it + 1 < spb);
  f32x4 bias1n = bias1;
  if (more) {      // the next slice's head weights and bias: requested a whole layer 1 ahead of their LDS store at the
                   // end of this pass (requested after the layer they waited ~1 k cycles in front of that store)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = min(tid + 256 * q, D * 16 - 1);
      w2pre[q] = *(const f32x4*)(np.w2 + (unsigned)((e >> 4) * HID + (ns + 1) * 64 + 4 * (e & 15)));
    }
    bias1n = *(const f32x4*)(np.b1 + (unsigned)((ns + 1) * 64 + wave * 16 + 4 * g));
  }
  // save H0 columns [64*ns, +64) of the trainable instances for the backward pass
  if (slot >= 0) {
    const int rl = tid >> 3;
    const int row = row0 + rl;
    if (row < B) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = ns * 64 + 4 * ((tid & 7) + 8 * j);
        if constexpr (BF16)
          *(bf16x4*)((__bf16*)h0g + (unsigned)((slot * MB + row) * HID + col)) = *(const bf16x4*)(H0b + rl * H0B_LD + col);
        else
          *(f32x4*)(h0g + (unsigned)((slot * MB + row) * HID + col)) = *(const f32x4*)(H0s + rl * H0_LD + col);
      }
    }
  }

  if (it == 0) STAMP(p, 8);
  // ---- layer 1: this wave computes H1[32][16 units]; A = W1 fragments (m = unit), B = H0 (n = row)
  {
    f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    if constexpr (BF16) {
      // all 16 operand reads of the tile first (one wait), then the 16 MFMAs back to back: written as read -> convert ->
      // MFMA per k-block the loop ran at one LDS latency + 8 conversions per pair of MFMAs (3.7 k cycles per slice at
      // 1 024 rows against 256 cycles of matrix work, profiles/r03_stamps_config5_1024_bf16.txt)
      bf16x8 b0[8], b1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        b0[j] = *(const bf16x8*)(H0b + l15 * H0B_LD + 32 * j + 8 * g);
        b1[j] = *(const bf16x8*)(H0b + (16 + l15) * H0B_LD + 32 * j + 8 * g);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {     // one bf16 MFMA per 32 k: lane (g) supplies k = 32 j + 8 g .. + 7 of both operands
        acc0 = MFMA_BF16(bwb[j], b0[j], acc0);
        acc1 = MFMA_BF16(bwb[j], b1[j], acc1);
        if ((j & 1) && more) {      // the next slice's fragments replace the two just used
          bwb[j - 1] = BWB_AT(n1 + 64, j - 1);
          bwb[j] = BWB_AT(n1 + 64, j);
        }
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const f32x4 a0 = *(const f32x4*)(H0s + l15 * H0_LD + 16 * ks + 4 * g);
        const f32x4 a1 = *(const f32x4*)(H0s + (16 + l15) * H0_LD + 16 * ks + 4 * g);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc0 = MFMA16(bw[ks][t], a0[t], acc0);
          acc1 = MFMA16(bw[ks][t], a1[t], acc1);
        }
        // more slices to come: the next slice's W1 fragments are requested into the registers whose MFMAs have just
        // been issued, four k-steps at a time — they arrive under the rest of this layer and the head phase
        if ((ks & 3) == 3 && more) {
#pragma unroll
          for (int k2 = ks - 3; k2 <= ks; ++k2)
            bw[k2] = *(const f32x4*)(np.w1 + (unsigned)((n1 + 64) * HID + 16 * k2 + 4 * g));
        }
      }
    }
    if (it == 0) STAMP(p, 9);
    f32x4 h0, h1;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      h0[reg] = fmaxf(acc0[reg] + bias1[reg], 0.f);
      h1[reg] = fmaxf(acc1[reg] + bias1[reg], 0.f);
    }
    if (drop) {   // hidden-1 units ns*64 + wave*16 + 4g .. +3 of rows l15 and 16 + l15
      const int word = ns * 2 + (wave >> 1), sh = (wave & 1) * 16 + 4 * g;
      const unsigned ba = Mk[256 + l15 * 8 + word] >> sh, bb_ = Mk[256 + (16 + l15) * 8 + word] >> sh;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        h0[reg] = ((ba >> reg) & 1u) ? h0[reg] * p.drop_scale : 0.f;
        h1[reg] = ((bb_ >> reg) & 1u) ? h1[reg] * p.drop_scale : 0.f;
      }
    }
    *(f32x4*)(H1s + l15 * T64_LD + wave * 16 + 4 * g) = h0;
    *(f32x4*)(H1s + (16 + l15) * T64_LD + wave * 16 + 4 * g) = h1;
  }
  if (it == 0) STAMP(p, 10);
  __syncthreads();
  if (it == 0) STAMP(p, 11);
  STAMP(p, 3);
  if (more) n1 += 64;

  {
    const int rl = tid >> 3;
    const int row = row0 + rl;
    const int sub = tid & 7;
    if (slot >= 0 && row < B) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int cl = 4 * (sub + 8 * j);
        st4<BF16>(h1g, (unsigned)((slot * MB + row) * HID + ns * 64 + cl), *(const f32x4*)(H1s + rl * T64_LD + cl));
      }
    }
    // ---- head partial sums over this block's 64 hidden-1 units (slice 0 also adds the bias)
    // thread (row rl, sub): units 4 sub..4 sub+3 and 32+4 sub..; its H1 values are read once, not once per dim
    const f32x4 ha = *(const f32x4*)(H1s + rl * T64_LD + 4 * sub);
    const f32x4 hb = *(const f32x4*)(H1s + rl * T64_LD + 32 + 4 * sub);
    if (D == 1) {
      const f32x4 wa = *(const f32x4*)(W2s + 4 * sub);
      const f32x4 wb = *(const f32x4*)(W2s + 32 + 4 * sub);
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(ha[e], wa[e], acc);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(hb[e], wb[e], acc);
      acc += __shfl_xor(acc, 1);
      acc += __shfl_xor(acc, 2);
      acc += __shfl_xor(acc, 4);
      if (ns == 0) acc += W2s[Dp * W2_LD];
      if (sub == 0 && row < B) {
        if (inst < 6) headsg[row * HEAD_LD + inst * NSPLIT + ns] = acc;
        else headsg[MB * HEAD_LD + row * NSPLIT + ns] = acc;           // a policy with one action dim
      }
    } else {
      // policy head on the matrix cores: partial[32 rows][Dp] = H1s[32][64] x W2s^T — wave w takes row tile w & 1
      // and the 16 action dims of tile w >> 1 (waves beyond Dp / 16 tiles idle), 16 dependent MFMAs over the block's
      // 64 units.  A = H1 (m = row, k = unit), B = W2 (k = unit, n = dim, zero rows beyond D).  (As scalar code the
      // policy instance was the forward's long pole: ~500 cycles per action dim.)
      if (16 * (wave >> 1) < Dp) {
        const int i = wave & 1, nt = wave >> 1;
        float a[16], b[16];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          a[ks] = H1s[(16 * i + l15) * T64_LD + 4 * ks + g];
          b[ks] = W2s[(16 * nt + l15) * W2_LD + 4 * ks + g];
        }
        f32x4 hacc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) hacc = MFMA16(a[ks], b[ks], hacc);
        const int dd = 16 * nt + l15;
        const float bias = (ns == 0) ? W2s[Dp * W2_LD + min(dd, D - 1)] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int prow_ = row0 + 16 * i + 4 * g + reg;
          if (dd < D && prow_ < B) headsg[MB * HEAD_LD + (prow_ * Aact + dd) * NSPLIT + ns] = hacc[reg] + bias;
        }
      }
    }
  }
  if (it == 0) STAMP(p, 12);
  if (!more) break;
  __syncthreads();      // every thread is done with this slice's H1s / W2s
  if (it == 0) STAMP(p, 13);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = tid + 256 * q;
    if (e < D * 16) *(f32x4*)(W2s + (e >> 4) * W2_LD + 4 * (e & 15)) = w2pre[q];
  }
  bias1 = bias1n;
  ++ns;
  }   // (the next slice's H1s / W2s writes are ordered before their readers by the barrier after its layer 1)
  STAMP(p, 4);
  RT_STAMP(p, 14, rt_entry_);
  RT_STAMP(p, 15, iql_realtime());

// Body of the update — included by iql_update_kernel and iql_update_group_kernel (iqlhip_kernels.h):
// ONE body for the single-agent kernel and its trainer-group form, so the arithmetic exists once.  blockIdx.x / gridDim.x
// are the block's index and grid size of ONE agent's launch in both (a group kernel's agent is blockIdx.y).
// In scope: template flags FROM_TABLE, PEER, LB, CLIP, the leading arguments q_*, `u` (UpdParams) and `step` (row of the
// scalar table and of the loss ring: 0 for iql_update_kernel, the bounded step index of a group launch).
// CLIP (iqlhip_set_grad_clip): q_clip[3] holds the optimizer groups' clip coefficients of this step.
  // XCD-affine element map: block (x = blockIdx & 7, q = blockIdx >> 3) — XCD x under the round-robin workgroup
  // dispatch — owns net x & 3, and of that net's arena segment the 64-float stripes of parity x >> 2: window q of 2 048
  // floats, 16 stripes of 16 threads.  The backward's blocks of net n run on XCDs n and n + 4 and a dW1 tile of column
  // parity h is written on XCD n + 4 h (W1 sits at the start of the segment, 4 stripes per row): the gradient is read
  // on the XCD that wrote it; the forward instances of net n (and the target copies') sit on XCDs n and n + 4 and read
  // the stripes their own XCD wrote, and the optimizer state is only ever touched by one XCD.
  const int ux = (int)(blockIdx.x & 7u), uq = (int)(blockIdx.x >> 3);
  const int net = ux & 3, uhalf = ux >> 2;
  // (segments are contiguous and 64-aligned: a net's segment ends where the next one begins, iqlhip_arena_layout)
  const long long seg_b = (long long)((net == 0) ? q_s0 : ((net == 1) ? q_s1 : ((net == 2) ? q_s2 : q_s3)));
  const long long seg_e = (long long)((net == 0) ? q_s1 : ((net == 1) ? q_s2 : ((net == 2) ? q_s3 : q_end)));
  const long long e = seg_b + (long long)uq * 2048 + (long long)((((int)threadIdx.x >> 4) * 2 + uhalf) * 64 + ((int)threadIdx.x & 15) * 4);
  if (e < seg_e) {
    // issue the state loads before the gradient sum so that all of them are in flight together — from the preloaded
    // arguments: nothing here waits for `u`
    f32x4 m = *(f32x4*)(q_m + e);
    f32x4 v = *(f32x4*)(q_v + e);
    f32x4 pw = *(f32x4*)(q_p + e);
    // W1 leads a segment (65 536 elements = 32 of the blocks' 2 048-float windows: the test is block-uniform)
    const bool early_g = !PEER && !LB && (q_flags & UPD_EARLY_G) != 0u && (e - seg_b) < 65536;
    f32x4 gr = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (early_g) gr = *(const f32x4*)(q_slab_a + e);
    float cf = 1.f;
    if (CLIP) cf = q_clip[(net == IQLHIP_NET_V) ? 0 : ((net == IQLHIP_NET_PI) ? 2 : 1)];
    __builtin_amdgcn_sched_barrier(0);      // (the loads above are issued BEFORE the argument fetch below is waited for)
    // every kernel-argument word the optimizer path uses, fetched in ONE batch of scalar loads (hipcc otherwise sinks
    // each load next to its first use: five dependent scalar-cache misses in front of the gradient loads).  ONE asm
    // statement for all of them: a volatile asm per word is ordered against the others and gets its own wait.
#define U64(x) ((unsigned long long)(x))
    asm volatile("" ::"s"(U64(u.L.net[0].seg_begin)), "s"(U64(u.L.net[1].seg_begin)), "s"(U64(u.L.net[2].seg_begin)),
                 "s"(U64(u.L.net[3].seg_begin)), "s"(U64(u.L.net[0].w0)), "s"(U64(u.L.net[1].w0)), "s"(U64(u.L.net[2].w0)),
                 "s"(U64(u.L.net[3].w0)), "s"(U64(u.L.net[0].b0)), "s"(U64(u.L.net[1].b0)), "s"(U64(u.L.net[2].b0)),
                 "s"(U64(u.L.net[3].b0)), "s"(u.L.net[0].k_in), "s"(u.L.net[1].k_in), "s"(u.L.net[2].k_in),
                 "s"(u.L.net[3].k_in), "s"(U64(u.slab_b_off[0])), "s"(U64(u.slab_b_off[1])), "s"(U64(u.slab_b_off[2])),
                 "s"(U64(u.slab_b_off[3])), "s"(U64(u.L.n_params)), "s"(U64(u.L.target_src)), "s"(U64((uintptr_t)u.params)),
                 "s"(U64((uintptr_t)u.target)), "s"(U64((uintptr_t)u.m)), "s"(U64((uintptr_t)u.v)),
                 "s"(U64((uintptr_t)u.slab_a)), "s"(U64((uintptr_t)u.slab_b)), "s"(U64((uintptr_t)u.flat_grads)),
                 "s"(U64((uintptr_t)u.sched)));
#undef U64

    const bool is_q = (net == IQLHIP_NET_Q1 || net == IQLHIP_NET_Q2);
    float* tp = u.target + (is_q ? (e - u.L.target_src) : 0);
    f32x4 t = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (is_q) t = *(f32x4*)tp;
    if (PEER) {
      // all ranks' contributions requested together (one fabric round trip), summed in rank order
      static_assert(IQLHIP_MAX_WORLD == 8, "load16_sys_x8");
      const NetWords nl = net_words(u, net);
      if (u.peer_direct && e >= nl.w0 && e < nl.b0 + HID) {
        // w0 / b0: every rank's <= 8 row-tile partial slabs, summed per rank in slab order (exactly slab_grad's sum,
        // i.e. what that rank's flatten kernel would have written), then over the ranks in rank order
        const long long stride = (long long)HID * nl.k_in + HID;
        const long long off = nl.slab_b_off + (e - nl.w0);
        gr = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < u.n_peer; ++r) {
          f32x4 pv[8];
          const float* pp[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) pp[j] = u.peer_slab_b[r] + off + (long long)min(j, u.n_rt - 1) * stride;
          load16_sys_x8(pv, pp);
          f32x4 gsum = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 8; ++j) if (j < u.n_rt) gsum += pv[j];
          gr = (r == 0) ? gsum : gr + gsum;
        }
      } else {
        f32x4 pv[8];
        const float* pp[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) pp[r] = u.peer_flat[min(r, u.n_peer - 1)] + e;
        load16_sys_x8(pv, pp);
        gr = pv[0];
#pragma unroll
        for (int r = 1; r < IQLHIP_MAX_WORLD; ++r) if (r < u.n_peer) gr += pv[r];
      }
    } else if (u.flat_grads) gr = *(const f32x4*)(u.flat_grads + e);
    else if (!early_g) gr = slab_grad<LB>(u, e, net);
    const int grp = (net == IQLHIP_NET_V) ? 0 : ((net == IQLHIP_NET_PI) ? 2 : 1);
    // (copy by value: a pointer that may address either the kernarg segment or global memory would make
    //  every access a flat load)
    iqlhip_step_scalars sc;
    if (FROM_TABLE) sc = u.sched[u.sched_idx + step];
    else sc = u.sc;
    const float gs = sc.grad_scale;
    const float step = -((grp == 0) ? sc.step_size[0] : ((grp == 1) ? sc.step_size[1] : sc.step_size[2]));
    const float bc2 = (grp == 0) ? sc.bc2_sqrt[0] : ((grp == 1) ? sc.bc2_sqrt[1] : sc.bc2_sqrt[2]);
    const float omb1 = sc.one_minus_beta1, b2 = sc.beta2, omb2 = sc.one_minus_beta2, eps = sc.eps;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // (the fused multiply-adds are spelled out: left to -ffp-contract the four instantiations of this kernel are free
      //  to fuse differently, and the exchange variants must stay bitwise equal to the plain one)
      // (CLIP: one separately rounded multiply by the group's coefficient — never contracted into the subtraction below)
      const float gk = CLIP ? __fmul_rn((gs == 1.f) ? gr[k] : gr[k] * gs, cf) : ((gs == 1.f) ? gr[k] : gr[k] * gs);
      m[k] = fmaf(omb1, gk - m[k], m[k]);
      v[k] = fmaf(omb2 * gk, gk, v[k] * b2);
      const float denom = sqrtf(v[k]) / bc2 + eps;
      pw[k] = fmaf(step, m[k] / denom, pw[k]);
    }
    *(f32x4*)(q_m + e) = m;
    *(f32x4*)(q_v + e) = v;
    *(f32x4*)(q_p + e) = pw;
    if (u.wsh) st4<true>((float*)u.wsh, (unsigned)e, pw);
    if (is_q) {
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = fmaf(u.tau, pw[k], u.one_minus_tau * t[k]);
      *(f32x4*)tp = t;
      if (u.tsh) st4<true>((float*)u.tsh, (unsigned)(e - u.L.target_src), t);
    }
    if (LB && u.wimg) {      // large-batch bf16 path: the operand images of W1 / W0 (W1 leads a net's segment)
      const NetWords nw = net_words(u, net);
      img_store4(u.wimg + (size_t)net * IMG_STRIDE, e, seg_b, nw.w0, nw.k_in, pw);
      if (is_q) img_store4(u.wimg + (size_t)(3 + net) * IMG_STRIDE, e, seg_b, nw.w0, nw.k_in, t);      // (nets 1, 2 -> slots 4, 5)
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float l[3];
    const float sc_ib = FROM_TABLE ? u.sched[u.sched_idx + step].inv_batch : u.sc.inv_batch;
    if (PEER && u.peer_direct) {
      // per rank the tail words its flatten kernel would have written (one chunk: loss_parts[k * 64]), summed in rank order
      const float ib = sc_ib;
      f32x4 t = (f32x4){0.f, 0.f, 0.f, 0.f};
      for (int r = 0; r < u.n_peer; ++r) {
        float s4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s4[k] = 0.f + __hip_atomic_load(u.peer_loss[r] + k * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const f32x4 tr = (f32x4){s4[0] * ib, (s4[1] * ib + s4[2] * ib) * 0.5f, s4[3] * ib, 0.f};
        t = (r == 0) ? tr : t + tr;
      }
      l[0] = t[0]; l[1] = t[1]; l[2] = t[2];
    } else if (PEER) {
      f32x4 t = load16_sys(u.peer_flat[0] + u.L.n_params);
      for (int r = 1; r < u.n_peer; ++r) t += load16_sys(u.peer_flat[r] + u.L.n_params);
      l[0] = t[0]; l[1] = t[1]; l[2] = t[2];
    } else if (u.flat_grads) {
      l[0] = u.flat_grads[u.L.n_params + 0];
      l[1] = u.flat_grads[u.L.n_params + 1];
      l[2] = u.flat_grads[u.L.n_params + 2];
    } else {
      float s[4];
      loss_words(u, s);
      const float ib = 1.f / (float)u.batch_rows;
      l[0] = s[0] * ib;                         // mean(w u^2)                        iql.py:302
      l[1] = (s[1] * ib + s[2] * ib) * 0.5f;    // (mse(q1,y) + mse(q2,y)) / 2        iql.py:508
      l[2] = s[3] * ib;                         // mean(exp_adv * bc)                 iql.py:534
    }
    u.losses[0] = l[0]; u.losses[1] = l[1]; u.losses[2] = l[2];
    if (u.losses_mirror) { u.losses_mirror[0] = l[0]; u.losses_mirror[1] = l[1]; u.losses_mirror[2] = l[2]; }
    if (u.done_flag) __hip_atomic_store(u.done_flag, u.done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (u.loss_ring) {
      const long long slot = (long long)u.ring_slot + step + (u.ring_hdr ? (long long)u.ring_hdr[HDR_BASE] : 0ll);
      *(float4*)(u.loss_ring + 4 * slot) = make_float4(l[0], l[1], l[2], 0.f);     // (host-mapped: one posted write)
    }
    if (u.adv_hdr) {      // the chunk is done: its successor finds its own per-launch values
      u.adv_hdr[HDR_POS] += (unsigned long long)u.adv_k * (unsigned long long)u.adv_rows;
      u.adv_hdr[HDR_DROP_STEP] += (unsigned long long)u.adv_k;
      u.adv_hdr[HDR_BASE] += (unsigned long long)u.adv_k;
      u.adv_hdr[HDR_XSTEP] += (unsigned long long)u.adv_k;
    }
  }

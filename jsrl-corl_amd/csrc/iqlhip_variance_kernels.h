// iqlhip_variance_kernels.h — one gradient step of the JSRL variance learner (iqlhip_var_step).
// Included by iqlhip.hip behind iqlhip_kernels.h and iqlhip_score_kernels.h (HID, H0_LD, MFMA16, NetPtrs, block_sum_256,
// score_l0).  Two scalar networks S -> 256 -> 256 -> 1 — mf (the value mean, net 0) and vf (the log-variance, net 1) — over
// a rollout of B <= VAR_MAX_ROWS consecutive environment steps, fp32 throughout:
//
//   iql_var_fwd_kernel    both nets over 32-row tiles (grid.y = net): mf on B + 1 rows (the B states and the bootstrap
//                         row, the last next-state), vf on B rows; head outputs, and the H0 / H1 tiles of the net that
//                         is going to be updated
//   iql_var_row_kernel    one block: the reverse recurrence of the sampled values (one lane, the reference's order and
//                         roundings), the clip and its gate, the per-row loss terms and their sum in a fixed order,
//                         the forward scan of the bootstrap row's gradient, the output-gradient column
//   iql_var_bwd_kernel    the chosen net's gradient: blocks 0..15 dW1 (16 output units each), blocks 16..31 dH0 of 16
//                         layer-0 units over all rows and from it dW0 / db0, block 32 dW2, db1, db2.  Every sum runs
//                         over the rows in a fixed order inside one wave or one thread: no atomics
//   iql_var_adam_kernel   torch's Adam on the net's segment of the arena (iql_update_kernel's operation order)
//   iql_var_pack_window_kernel   the packed block from B consecutive rows of a packed replay buffer, the start row an
//                         argument or drawn in the kernel (iqlhip_var_train_steps; DESIGN.md 6l "From a replay buffer")
//
// The kernels are templates of one unused parameter and read neither gridDim nor blockDim, as the scoring group kernels
// (iqlhip_score_kernels.h: why): they are emitted behind every other kernel of the code object.
#pragma once

#define VAR_MAX_ROWS 1024        // B of a step
#define VAR_LD 1040              // rows of the per-row scratch: B + 1 rounded up to whole 16-row MFMA tiles
#define VAR_GAMMA 0.99f          // variance_learner.py GAMMA
#define VAR_CLIP_LO 1e-4f
#define VAR_CLIP_HI 1e8f

struct VarFwdParams {
  NetPtrs net[2];                // mf, vf: the fp32 masters of the bound arena
  const float* x;                // the packed block's rows [B + 1][S]: B states, then the last next-state
  int S;
  int rows0, rows1;              // rows each net runs on: B + 1, B
  int keep;                      // the net whose activations are kept for the backward (-1: none)
  float* h0;                     // [VAR_LD][256] post-ReLU activations of `keep`
  float* h1;
  float* out;                    // [2][VAR_LD] head outputs
};

// blockIdx.x = 32-row tile, blockIdx.y = net.  Layer 0 and layer 1 are score_l0 (weights from the cache hierarchy, the
// rows from the packed block / the H0 tile in LDS); a lane's accumulators are 4 consecutive units of one row.  Rows past
// the net's last repeat it; their results are never stored.  The head: per lane 16 units of a row in a fixed order, then
// the row's 16 lane partials (4 waves x 4 lane groups) added in order by one thread.
template <int = 0> __global__ __launch_bounds__(256) void iql_var_fwd_kernel(VarFwdParams p) {
  const int tile = blockIdx.x, net = blockIdx.y;
  const int n = net ? p.rows1 : p.rows0;
  if (tile * 32 >= n) return;                 // (block-uniform: before any barrier)
  const NetPtrs np = net ? p.net[1] : p.net[0];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int S = p.S;
  const bool keep = p.keep == net;
  __shared__ __attribute__((aligned(16))) float H0s[32 * H0_LD];
  __shared__ float part[16 * 32];

  const int row0 = tile * 32 + l15, row1 = row0 + 16;
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  score_l0(acc, np.w0, p.x + (size_t)min(row0, n - 1) * S, p.x + (size_t)min(row1, n - 1) * S, S, (S + 3) >> 2, wave, l15, g);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int unit = wave * 64 + ct * 16 + 4 * g;
    const f32x4 bias0 = *(const f32x4*)(np.b0 + unit);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      f32x4 h;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) h[reg] = fmaxf(acc[rt][ct][reg] + bias0[reg], 0.f);
      *(f32x4*)(H0s + (rt * 16 + l15) * H0_LD + unit) = h;
      const int row = rt ? row1 : row0;
      if (keep && row < n) *(f32x4*)(p.h0 + (size_t)row * HID + unit) = h;
    }
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  score_l0(acc, np.w1, H0s + l15 * H0_LD, H0s + (16 + l15) * H0_LD, HID, HID / 4, wave, l15, g);
  float hp[2] = {0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int unit = wave * 64 + ct * 16 + 4 * g;
    const f32x4 bias1 = *(const f32x4*)(np.b1 + unit);
    const f32x4 w2 = *(const f32x4*)(np.w2 + unit);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      f32x4 h;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        h[reg] = fmaxf(acc[rt][ct][reg] + bias1[reg], 0.f);
        hp[rt] = fmaf(h[reg], w2[reg], hp[rt]);
      }
      const int row = rt ? row1 : row0;
      if (keep && row < n) *(f32x4*)(p.h1 + (size_t)row * HID + unit) = h;
    }
  }
  part[(wave * 4 + g) * 32 + l15] = hp[0];
  part[(wave * 4 + g) * 32 + 16 + l15] = hp[1];
  __syncthreads();
  if (tid < 32) {
    const int row = tile * 32 + tid;
    if (row < n) {
      float s = part[tid];
#pragma unroll
      for (int i = 1; i < 16; ++i) s += part[i * 32 + tid];
      p.out[net * VAR_LD + row] = s + np.b2[0];
    }
  }
}

// ---------------------------------------------------------------------------
struct VarRowParams {
  const float* out;              // [2][VAR_LD] head outputs: pred (row B: the bootstrap value), s
  const float* rew;              // [B] rewards of the packed block
  const float* nd;               // [B] next-done flags, 0 or 1
  int B;
  int which;                     // the net whose output gradient is formed: 0 mf, 1 vf, -1 none
  int aligned;                   // 0: the reference's rewards[t - 1] (row 0 takes rewards[B - 1]); 1: rewards[t]
  float* vals;                   // samp | pred | var, each [B] at stride VAR_LD (the handle's host-mapped landing words)
  float* vals2;                  // the same at stride B for a caller's [3][B] array, or null
  float* dy;                     // [VAR_LD] the output-gradient column (mf: B + 1 rows; vf: B rows)
  float* loss;                   // [1]
};

// One block of 256 threads.  samp[t] = reward + (GAMMA * next) * (1 - next_done[t]), every operation rounded on its own,
// walked from t = B - 1 down by lane 0.  loss = mean(0.5 * (log(var) + d^2 / var)), d = pred - samp: a thread adds its
// rows t = tid, tid + 256, ... in order, the 256 sums are added by block_sum_256's fixed tree.  The total gradient on
// samp[t + 1] is its direct term -d / (var B) plus GAMMA * nnt[t] times the total on samp[t]: a forward scan by lane 0,
// whose last value times GAMMA * nnt[B - 1] is the bootstrap row's output gradient (the reference does not detach it).
template <int = 0> __global__ __launch_bounds__(256) void iql_var_row_kernel(VarRowParams p) {
#pragma clang fp contract(off)
  __shared__ float samp[VAR_MAX_ROWS], nnt[VAR_MAX_ROWS], rw[VAR_MAX_ROWS], gdir[VAR_MAX_ROWS];
  __shared__ float red[4];
  const int tid = threadIdx.x, B = p.B;
  for (int t = tid; t < B; t += 256) {
    nnt[t] = 1.f - p.nd[t];
    rw[t] = p.rew[p.aligned ? t : (t == 0 ? B - 1 : t - 1)];
  }
  __syncthreads();
  if (tid == 0) {
    float next = p.out[B];
    for (int t = B - 1; t >= 0; --t) {
      const float gn = VAR_GAMMA * next;
      const float s = rw[t] + gn * nnt[t];
      samp[t] = s;
      next = s;
    }
  }
  __syncthreads();
  const float inv_b = 1.f / (float)B;
  float lsum = 0.f;
  for (int t = tid; t < B; t += 256) {
    const float pred = p.out[t], s = p.out[VAR_LD + t];
    const float e = expf(s);
    const bool open = (e >= VAR_CLIP_LO) && (e <= VAR_CLIP_HI);
    const float var = fminf(fmaxf(e, VAR_CLIP_LO), VAR_CLIP_HI);
    const float d = pred - samp[t];
    const float q = (d * d) / var;
    lsum = lsum + 0.5f * (logf(var) + q);
    const float gp = (d / var) * inv_b;
    gdir[t] = -gp;
    p.vals[t] = samp[t];
    p.vals[VAR_LD + t] = pred;
    p.vals[2 * VAR_LD + t] = var;
    if (p.vals2) {
      p.vals2[t] = samp[t];
      p.vals2[B + t] = pred;
      p.vals2[2 * B + t] = var;
    }
    if (p.which == 0) p.dy[t] = gp;
    else if (p.which == 1) p.dy[t] = open ? (0.5f * (1.f - q)) * inv_b : 0.f;
  }
  const float total = block_sum_256(lsum, red);      // (its barriers publish gdir)
  if (tid == 0) {
    p.loss[0] = total / (float)B;
    if (p.which == 0) {
      float G = gdir[0];
      for (int t = 1; t < B; ++t) G = gdir[t] + (VAR_GAMMA * nnt[t - 1]) * G;
      p.dy[B] = (VAR_GAMMA * nnt[B - 1]) * G;
    }
  }
}

// ---------------------------------------------------------------------------
struct VarBwdParams {
  NetPtrs np;                    // the net being updated
  const float* x;                // [n][S] rows of the packed block
  int S;
  int n;                         // rows: B + 1 (mf) or B (vf)
  const float* h0;               // [VAR_LD][256]
  const float* h1;
  const float* dy;               // [VAR_LD]
  float* dh0;                    // [VAR_LD][256] scratch: dH0 (pre-activation), written and read inside one block
  float* grad;                   // the net's gradient, laid out as its segment of the arena
  unsigned g_w1, g_w0, g_b0, g_b1, g_w2, g_b2;
};

#define VAR_BWD_BLOCKS 33
// dH1 (pre-activation) of a row and a unit is never stored: dy[t] * W2[u] where H1[t][u] > 0, formed where it is an
// operand.  Rows t >= n contribute exact zeros: the gradient-side operand is zero and the other side is read at a
// clamped, valid row (finite x 0 = 0).
template <int = 0> __global__ __launch_bounds__(256) void iql_var_bwd_kernel(VarBwdParams p) {
  const int blk = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int n = p.n, S = p.S;
  const NetPtrs np = p.np;
  __shared__ float W2s[HID];
  W2s[tid] = np.w2[tid];
  __syncthreads();

  if (blk < 16) {
    // ---- dW1[u][k] = sum_t dH1[t][u] H0[t][k]: 16 units u of this block, wave w the columns k = 64 w .. 64 w + 63.
    // A = dH1^T (m = unit, k = row), B = H0 (k = row, n = column)
    const int u = blk * 16 + l15;
    const float w2u = W2s[u];
    f32x4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nts = (n + 3) >> 2;
#pragma unroll 4
    for (int ts = 0; ts < nts; ++ts) {
      const int tt = 4 * ts + g, tc = min(tt, n - 1);
      const float h1v = p.h1[(size_t)tc * HID + u];
      const float a = (tt < n && h1v > 0.f) ? p.dy[tc] * w2u : 0.f;
      float b[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) b[ct] = p.h0[(size_t)tc * HID + wave * 64 + ct * 16 + l15];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = MFMA16(a, b[ct], acc[ct]);
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        p.grad[p.g_w1 + (unsigned)((blk * 16 + 4 * g + reg) * HID + wave * 64 + ct * 16 + l15)] = acc[ct][reg];
  } else if (blk < 32) {
    // ---- dH0[t][k] for the 16 layer-0 units k = k0 .. k0 + 15 and every row: sum_u dH1[t][u] W1[u][k], masked by
    // H0[t][k] > 0.  A = W1^T (m = unit k, k = unit u: the same for every row tile, kept in registers), B = dH1^T
    // (k = unit u, n = row).  Wave w takes the 16-row tiles w, w + 4, ...
    const int k0 = (blk - 16) * 16;
    float a[64];
#pragma unroll
    for (int us = 0; us < 64; ++us) a[us] = np.w1[(unsigned)((4 * us + g) * HID + k0 + l15)];
    const int nt16 = (n + 15) >> 4;
    for (int tile = wave; tile < nt16; tile += 4) {
      const int tt = tile * 16 + l15, tc = min(tt, n - 1);
      const float dyt = (tt < n) ? p.dy[tc] : 0.f;
      const float* h1r = p.h1 + (size_t)tc * HID;
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll      // (whole: a[] is indexed by constants and stays in registers)
      for (int us = 0; us < 64; ++us) {
        const int uu = 4 * us + g;
        const float b = (h1r[uu] > 0.f) ? dyt * W2s[uu] : 0.f;
        acc = MFMA16(a[us], b, acc);
      }
      // acc[reg] = dH0[row tile * 16 + l15][k0 + 4 g + reg]
      const f32x4 h0v = *(const f32x4*)(p.h0 + (size_t)tc * HID + k0 + 4 * g);
      f32x4 d;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) d[reg] = (tt < n && h0v[reg] > 0.f) ? acc[reg] : 0.f;
      *(f32x4*)(p.dh0 + (size_t)tt * HID + k0 + 4 * g) = d;      // (tt < nt16 * 16 <= VAR_LD)
    }
    __syncthreads();      // the block's own dH0 columns, rows 0 .. 16 nt16 - 1, are visible to all its waves
    // ---- dW0[k][j] = sum_t dH0[t][k] X[t][j], and db0[k] as column j = S of ones.  A = dH0^T (m = unit, k = row),
    // B = X (k = row, n = column).  Wave w takes the column tiles w, w + 4, ...
    const int njt = (S + 1 + 15) >> 4;
    const int nts = (n + 3) >> 2;
    for (int jt = wave; jt < njt; jt += 4) {
      const int jc = jt * 16 + l15;
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int ts = 0; ts < nts; ++ts) {
        const int tt = 4 * ts + g, tc = min(tt, n - 1);
        const float av = p.dh0[(size_t)tt * HID + k0 + l15];
        const float xv = p.x[(size_t)tc * S + min(jc, S - 1)];
        const float b = (jc < S) ? xv : ((jc == S) ? 1.f : 0.f);
        acc = MFMA16(av, b, acc);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int k = k0 + 4 * g + reg;
        if (jc < S) p.grad[p.g_w0 + (unsigned)(k * S + jc)] = acc[reg];
        else if (jc == S) p.grad[p.g_b0 + (unsigned)k] = acc[reg];
      }
    }
  } else {
    // ---- thread u: dW2[u] = sum_t dy[t] H1[t][u], db1[u] = W2[u] sum_{t: H1[t][u] > 0} dy[t]; db2 = sum_t dy[t]
    float sw = 0.f, sb = 0.f, s2 = 0.f;
    for (int t = 0; t < n; ++t) {
      const float d = p.dy[t], h = p.h1[(size_t)t * HID + tid];
      sw = fmaf(d, h, sw);
      sb += (h > 0.f) ? d : 0.f;
      s2 += d;
    }
    p.grad[p.g_w2 + tid] = sw;
    p.grad[p.g_b1 + tid] = sb * W2s[tid];
    if (tid == 0) p.grad[p.g_b2] = s2;
  }
}

// ---------------------------------------------------------------------------
// torch.optim.Adam's defaults on n words (the net's whole segment: its padding words have zero gradients and stay zero).
// step_neg = -lr / (1 - beta1^t), bc2 = sqrt(1 - beta2^t): float64 on the host; eps is added behind the division by bc2.
template <int = 0> __global__ __launch_bounds__(256) void iql_var_adam_kernel(float* pw, float* m, float* v, const float* gr, int n,
                                                                             float step_neg, float bc2, float omb1, float b2,
                                                                             float omb2, float eps) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  const float gk = gr[i];
  const float mk = fmaf(omb1, gk - m[i], m[i]);
  const float vk = fmaf(omb2 * gk, gk, v[i] * b2);
  const float denom = sqrtf(vk) / bc2 + eps;
  m[i] = mk;
  v[i] = vk;
  pw[i] = fmaf(step_neg, mk / denom, pw[i]);
}

// ---------------------------------------------------------------------------
struct VarPackParams {
  const float* rows;             // packed replay rows [s | a | s' | r | d | pad] of stride ld
  long long ld;
  long long start;               // the window's first row (the eager form)
  long long last_start;          // size - B: the largest start whose window stays inside the buffer
  unsigned long long seed, j;    // DRAWN: index j of the index stream under `seed` at counter offset 0
  unsigned long long span;       // DRAWN: size - B + 1 values, or the length of `starts`
  const long long* starts;       // DRAWN: a list the draw indexes, or null
  long long* start_out;          // DRAWN: this update's word of the start ring
  int S, A, B;
  float* out;                    // the packed block: [B][S] states | [S] last next-state | [B] rewards | [B] next-dones
};

// Thread e = (t, c) of (B + 1) x (S + 2): t < B copies column c of row start + t — c < S a state word, c = S the reward,
// c = S + 1 the done flag (the buffer stores real_done: run_episodes' next_dones) —, t = B copies word c < S of the
// last row's next-state.  Consecutive lanes read consecutive words of a row.  Row offsets are 64-bit: start * ld floats
// passes 2^31 and 2^32 bytes on a 10 M-row buffer.  DRAWN: every thread draws the start itself (draw_index, as
// gather_rows_drawn: ~150 ALU instructions instead of a dependent load); an entry of `starts` is clamped into
// [0, last_start], so that no list can send a read outside the buffer.
template <bool DRAWN> __global__ __launch_bounds__(256) void iql_var_pack_window_kernel(VarPackParams p) {
  const int S = p.S, B = p.B, W = S + 2;
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;      // (B + 1) * W <= 1025 * 129
  if (e >= (B + 1) * W) return;
  long long start = p.start;
  if (DRAWN) {
    start = draw_index(p.seed, 0ull, p.j, p.span);
    if (p.starts) start = min(max(p.starts[start], 0ll), p.last_start);
    if (e == 0) *p.start_out = start;
  }
  const int t = e / W, c = e - t * W;
  const int r = 2 * S + p.A;
  if (t < B) {
    const float* row = p.rows + (start + (long long)t) * p.ld;
    if (c < S) p.out[t * S + c] = row[c];
    else if (c == S) p.out[(B + 1) * S + t] = row[r];
    else p.out[(B + 1) * S + B + t] = row[r + 1];
  } else if (c < S) {
    p.out[B * S + c] = p.rows[(start + (long long)(B - 1)) * p.ld + (S + p.A + c)];
  }
}

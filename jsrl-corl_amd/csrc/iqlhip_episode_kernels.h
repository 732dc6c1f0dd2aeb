// iqlhip_episode_kernels.h — per-row episode spans, returns and return-to-go (include/iqlhip.h
// iqlhip_rows_episode_returns).  Included by iqlhip.hip behind every other kernel of the library (the
// existing kernels keep their places in the code object); needs iqlhip_kernels.h (RR_TILE, RR_MAX_BLOCKS,
// rr_block_scan_max, iql_rr_scan_partials_kernel).
//
// Everything is defined in integers and float64 (the header states the arithmetic), so a CPU restatement agrees to the
// bit.  n packed rows [s | a | s' | r | d | pad] from row0, in storage order; i is 0-based in the range.
//   1. iql_ep_break_kernel: flag[i] = d[i] != 0, or (RULE) i + 1 < n and sum_c (double)dlt_c^2 > tol^2 with
//      dlt_c = s[i+1][c] - s'[i][c] in float32 — Cal-QL's norm(obs[t+1] - next_obs[t]) > 1e-6.
//   2. prev[i] = max over j <= i of (flag[j] ? j : -1): the three plain launches of the reward ingest's scan (a partial
//      per 256-row tile, iql_rr_scan_partials_kernel over the partials, every tile rescanned on its carry), over the
//      flag bytes instead of the done column.  No block waits for another one.
//      p(i) = prev[i - 1], o = i - p(i) - 1;  row i ends an episode iff prev[i] == i || (o + 1) % T == 0 ||
//      (KEEP_TAIL && i == n - 1), and that episode starts at p(i) + 1 + (o / T) * T.
//   3. iql_ep_walk_kernel: the thread of a row that ends an episode walks its at most T rewards forward (ep_return, the
//      sum of iql_rr_episode_kernel) and backward (return_to_go), in order; it writes ep_return at its own row only.
//   4. iql_ep_rows_kernel: row-parallel and coalesced — every row finds its episode's last row (prev is monotone: the
//      first k >= i with prev[k] >= i is the next break, a binary search over at most T entries that the lanes of a
//      wave share) and writes ep_first / ep_last, reads ep_return from the last row's slot, and zeroes tail rows.
#pragma once

#define EP_KEEP_TAIL 1                  // IQLHIP_EP_KEEP_TAIL
#define EP_LANES 16                     // lanes per row of the discontinuity rule: a wave reads 4 rows' columns at a time
#define EP_BREAK_MAX_BLOCKS 8192

// RULE = false: one thread per row reads the done column.  RULE = true: EP_LANES lanes per row; lane g takes columns
// g, g + 16, ... of s[i+1] and s'[i] (consecutive lanes, consecutive floats: a wave reads whole column blocks of four
// rows), then the squares are added in float64 in ascending column order — every lane of the row's group adds the same
// 16 shuffled values one after the other, so the order does not depend on the lane layout.
template <bool RULE>
__global__ __launch_bounds__(RR_TILE) void iql_ep_break_kernel(const float* __restrict__ rows, long long ld, int S, int A,
                                                               long long row0, long long n, double tol2,
                                                               unsigned char* __restrict__ flag) {
#pragma clang fp contract(off)
  const int dcol = 2 * S + A + 1;
  if (!RULE) {
    for (long long i = (long long)blockIdx.x * RR_TILE + threadIdx.x; i < n; i += (long long)gridDim.x * RR_TILE)
      flag[i] = rows[(row0 + i) * ld + dcol] != 0.f;
    return;
  }
  const int g = threadIdx.x & (EP_LANES - 1);
  const long long per_block = RR_TILE / EP_LANES;
  const long long rounds = (n + per_block - 1) / per_block;
  for (long long b = blockIdx.x; b < rounds; b += gridDim.x) {        // (uniform trip count: every lane shuffles)
    const long long i = b * per_block + (threadIdx.x / EP_LANES);
    const bool row_ok = i < n, has_next = i + 1 < n;
    const float* cur = rows + (row0 + (row_ok ? i : 0)) * ld;
    const float* nxt = cur + ld;
    double ss = 0.0;
    for (int c0 = 0; c0 < S; c0 += EP_LANES) {
      const int c = c0 + g;
      float dlt = 0.f;
      if (has_next && c < S) dlt = nxt[c] - cur[S + A + c];
      const int m = min(EP_LANES, S - c0);
      for (int k = 0; k < m; ++k) {
        const double v = (double)__shfl(dlt, k, EP_LANES);
        const double sq = v * v;
        ss = ss + sq;
      }
    }
    if (row_ok && g == 0) flag[i] = (cur[dcol] != 0.f) || (has_next && ss > tol2);
  }
}

__device__ __forceinline__ long long ep_break_or_minus1(const unsigned char* flag, long long n, long long i) {
  return (i < n && flag[i]) ? i : -1;
}

// partial[t] = the last break of tile t (-1: none)
__global__ __launch_bounds__(RR_TILE) void iql_ep_scan_reduce_kernel(const unsigned char* __restrict__ flag, long long n,
                                                                     long long ntiles, long long* partial) {
  __shared__ long long s_w[4];
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    long long v = ep_break_or_minus1(flag, n, t * RR_TILE + threadIdx.x);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long u = __shfl_xor(v, o, 64); if (u > v) v = u; }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partial[t] = max(max(s_w[0], s_w[1]), max(s_w[2], s_w[3]));
    __syncthreads();
  }
}

// prev[i] = the last break <= i of the whole range (-1: none); partial: scanned by iql_rr_scan_partials_kernel
__global__ __launch_bounds__(RR_TILE) void iql_ep_scan_apply_kernel(const unsigned char* __restrict__ flag, long long n,
                                                                    long long ntiles, const long long* partial,
                                                                    long long* prev) {
  __shared__ long long s_w[4];
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * RR_TILE + threadIdx.x;
    long long v = rr_block_scan_max(ep_break_or_minus1(flag, n, i), s_w);
    const long long carry = t ? partial[t - 1] : -1;
    if (carry > v) v = carry;
    if (i < n) prev[i] = v;
  }
}

// One thread per row; the thread of a row that ends an episode walks that episode.  ep_return (may be NULL): the float32
// rewards added in float64 from 0.0, first row to last, written at the END ROW only (iql_ep_rows_kernel hands it to the
// other rows).  rtg (may be NULL): G[last] = r[last], G[j] = r[j] + discount * G[j+1] downwards, product and sum rounded
// separately, written at every row of the episode; with `sparse` an episode whose last reward equals sparse_value gets
// r[last] / (1 - discount) on all its rows instead.  Eight loads in flight per thread, the arithmetic in row order.
// *episodes += the number of episodes (one integer atomic per block).
__global__ __launch_bounds__(RR_TILE) void iql_ep_walk_kernel(const float* __restrict__ rows, long long ld, int rcol,
                                                              long long row0, long long n, long long ntiles, long long T,
                                                              int keep_tail, double discount, int sparse,
                                                              double sparse_value, const long long* __restrict__ prev,
                                                              double* __restrict__ ep_return, double* __restrict__ rtg,
                                                              unsigned long long* episodes) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_cnt[4];
  unsigned long long cnt = 0;
  const float* r = rows + row0 * ld + rcol;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * RR_TILE + threadIdx.x;
    if (i >= n) continue;
    const long long p = i ? prev[i - 1] : -1;
    const long long o = i - p - 1;
    if (prev[i] != i && (o + 1) % T != 0 && !(keep_tail && i == n - 1)) continue;
    ++cnt;
    const long long first = p + 1 + (o / T) * T;
    if (ep_return) {
      double ret = 0.0;
      long long j = first;
      for (; j + 8 <= i + 1; j += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = r[(j + k) * ld];
#pragma unroll
        for (int k = 0; k < 8; ++k) ret += (double)v[k];
      }
      for (; j <= i; ++j) ret += (double)r[j * ld];
      ep_return[i] = ret;
    }
    if (rtg) {
      const double r_last = (double)r[i * ld];
      if (sparse && r_last == sparse_value) {
        const double g = r_last / (1.0 - discount);
        for (long long j = first; j <= i; ++j) rtg[j] = g;
      } else {
        double g = r_last;
        rtg[i] = g;
        long long j = i - 1;
        for (; j - 7 >= first; j -= 8) {
          float v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = r[(j - k) * ld];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const double dg = discount * g;
            g = (double)v[k] + dg;
            rtg[j - k] = g;
          }
        }
        for (; j >= first; --j) {
          const double dg = discount * g;
          g = (double)r[j * ld] + dg;
          rtg[j] = g;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (total) atomicAdd(episodes, total);
  }
}

// One thread per row, coalesced: the row's episode span, ep_return from its episode's end row, zeros on tail rows.
// The episode of row i starts at first = p + 1 + (o / T) * T and ends at the first break in [i, first + T - 1], else at
// first + T - 1 (the length rule), else — the range ends before either — at n - 1 with KEEP_TAIL or not at all.
// ep_return is written at rows that end no episode only, and read at rows that end one only: no row is both.
__global__ __launch_bounds__(RR_TILE) void iql_ep_rows_kernel(long long n, long long T, int keep_tail,
                                                              const long long* __restrict__ prev, double* ep_return,
                                                              double* __restrict__ rtg, long long* __restrict__ ep_first,
                                                              long long* __restrict__ ep_last) {
  for (long long i = (long long)blockIdx.x * RR_TILE + threadIdx.x; i < n; i += (long long)gridDim.x * RR_TILE) {
    const long long p = i ? prev[i - 1] : -1;
    const long long o = i - p - 1;
    long long first = p + 1 + (o / T) * T;
    const long long cap = (T - 1 < n - 1 - first) ? first + T - 1 : n - 1;       // min(first + T - 1, n - 1), no overflow
    long long last;
    if (prev[cap] >= i) {                  // a break in [i, cap]: the first k with prev[k] >= i
      long long lo = i, hi = cap;
      while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (prev[mid] >= i) hi = mid; else lo = mid + 1;
      }
      last = lo;
    } else if (cap - first == T - 1 || keep_tail) {
      last = cap;
    } else {
      first = last = -1;
    }
    if (ep_first) ep_first[i] = first;
    if (ep_last) ep_last[i] = last;
    if (last < 0) {
      if (ep_return) ep_return[i] = 0.0;
      if (rtg) rtg[i] = 0.0;
    } else if (ep_return && last != i) {
      ep_return[i] = ep_return[last];
    }
  }
}

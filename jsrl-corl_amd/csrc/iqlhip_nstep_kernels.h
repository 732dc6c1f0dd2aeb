// iqlhip_nstep_kernels.h — n-step rows derived from packed one-step rows (include/iqlhip.h iqlhip_rows_nstep,
// iqlhip_rows_nstep_ring, iqlhip_online_step_nstep).  Included by iqlhip.hip behind every other kernel of
// the library (the existing kernels keep their places in the code object); needs iqlhip_kernels.h (f32x4).
//
// A derived row is a one-step row the unchanged step kernels read as a k-step transition: s, a and the pad columns of
// row i, s' of row m, r = the discounted reward sum over rows i .. m, d = d[m] or 1 - discount^(k - 1).  The header
// states the arithmetic (integers and float64, fp contract off), so a CPU restatement agrees to the bit.
//
// Both kernels are row-parallel: NS_LANES lanes own one row (a wave: four rows).  Lane g of the group loads r and d of
// row i + g (+ 16 per round, at most NS_ROUNDS rounds: horizon <= 64), a ballot finds the first row that stops the
// chain, every lane of the group then runs the same Horner recurrence over the shuffled rewards, and the group copies the
// row in 16-byte pieces (lane g: pieces g, g + 16, ...; consecutive lanes, consecutive pieces).  A row only reads the
// source store and only writes its own derived row: no block waits for another one, plain vector stores, no atomics.
#pragma once

#define NS_LANES 16
#define NS_MAX_HORIZON 64               // IQLHIP_NSTEP_MAX_HORIZON
#define NS_ROUNDS (NS_MAX_HORIZON / NS_LANES)
#define NS_ROWS_PER_BLOCK (256 / NS_LANES)
#define NS_MAX_BLOCKS 8192

struct NstepArgs {
  const float* src;                     // packed one-step rows
  float* dst;                           // derived rows, the same positions
  long long src_ld, dst_ld;
  int S, A;
  int q;                                // 16-byte pieces of a row that are copied: iqlhip_row_stride(S, A) / 4
  int horizon, rounds;                  // rounds = ceil(horizon / NS_LANES)
  double discount;
  unsigned char* steps;                 // k per row (NULL: not wanted)
};

// The store position of logical row j of the range: build form row0 + j; ring form (base + j) mod cap with base the
// position of the oldest row (j < size <= cap, base < cap: one conditional subtraction).
template <bool RING>
__device__ __forceinline__ long long ns_pos(long long j, long long base, long long cap) {
  const long long p = base + j;
  return (RING && p >= cap) ? p - cap : p;
}

// Row i of a range of n logical rows (row_ok: i < n; every lane of the wave runs this, whole groups idle).
//   build form: ep_last (NULL: none) bounds the chain, relative to the range.
//   ring form:  ends[position] != 0 stops the chain behind that row.  newest_row != NULL (the fused online call): logical
//               row n - 1 is not in the store yet — it is read from newest_row (host-mapped), its end byte is newest_end,
//               and the group of row n - 1 stores both into raw_out / ends.
template <bool RING>
__device__ __forceinline__ void ns_row(const NstepArgs& a, long long base, long long cap, long long n, long long i, bool row_ok,
                                       const long long* __restrict__ ep_last, unsigned char* ends,
                                       const float* __restrict__ newest_row, int newest_end, float* raw_out) {
#pragma clang fp contract(off)
  const int g = threadIdx.x & (NS_LANES - 1);
  const int grp_bit = threadIdx.x & 48;                   // the group's first bit in the wave's ballot
  const int rcol = 2 * a.S + a.A, spcol = a.S + a.A;
  long long L = n - 1;
  if (a.horizon - 1 < L - i) L = i + a.horizon - 1;       // min(i + horizon - 1, n - 1)
  if (!RING && ep_last && row_ok) {
    long long e = ep_last[i];
    if (e >= 0) {                                         // (an entry outside [i, n - 1] is clamped into it)
      if (e < i) e = i;
      if (e < L) L = e;
    }
  }
  float rv[NS_ROUNDS], dv[NS_ROUNDS];
  int first = -1;                                         // offset from i of the first row that stops the chain
#pragma unroll
  for (int t = 0; t < NS_ROUNDS; ++t) {
    rv[t] = 0.f;
    dv[t] = 0.f;
    if (t < a.rounds) {                                   // (uniform: every lane votes)
      const long long j = i + t * NS_LANES + g;
      bool stop = false;
      if (row_ok && j <= L) {
        const bool fresh = newest_row && j == n - 1;
        const long long pj = ns_pos<RING>(j, base, cap);
        const float* p = fresh ? newest_row : a.src + pj * a.src_ld;
        rv[t] = p[rcol];
        dv[t] = p[rcol + 1];
        stop = dv[t] != 0.f;
        if (RING) stop = stop || (fresh ? newest_end != 0 : ends[pj] != 0);
      }
      const unsigned hits = (unsigned)(__ballot(stop) >> grp_bit) & 0xFFFFu;
      if (first < 0 && hits) first = t * NS_LANES + __ffs(hits) - 1;
    }
  }
  const int mo = first >= 0 ? first : (int)(L - i);       // m - i, in [0, horizon - 1]
  // G = r[m], then G = r[j] + discount * G for j = m - 1 .. i; the same order in every lane of the group
  double G = 0.0;
  float dm = 0.f;
#pragma unroll
  for (int t = NS_ROUNDS - 1; t >= 0; --t) {
    if (t < a.rounds) {
      const int k_hi = min(NS_LANES, a.horizon - t * NS_LANES) - 1;
      for (int k = k_hi; k >= 0; --k) {                   // (uniform trip count: every lane shuffles)
        const float r = __shfl(rv[t], k, NS_LANES);
        const float d = __shfl(dv[t], k, NS_LANES);
        const int o = t * NS_LANES + k;
        if (o == mo) {
          G = (double)r;
          dm = d;
        } else if (o < mo) {
          const double dg = a.discount * G;
          G = (double)r + dg;
        }
      }
    }
  }
  if (!row_ok) return;
  float dval = dm;
  if (dm == 0.f) {                                        // 1 - discount^(k - 1), the product built one factor at a time
    double c = 1.0;
    for (int t = 0; t < mo; ++t) c = c * a.discount;
    dval = (float)(1.0 - c);
  }
  const float Gf = (float)G;
  const long long pi = ns_pos<RING>(i, base, cap), pm = ns_pos<RING>(i + mo, base, cap);
  const bool i_fresh = newest_row && i == n - 1;
  const float* si = i_fresh ? newest_row : a.src + pi * a.src_ld;
  const float* sm = (newest_row && i + mo == n - 1) ? newest_row : a.src + pm * a.src_ld;
  float* di = a.dst + pi * a.dst_ld;
  for (int c4 = g; c4 < a.q; c4 += NS_LANES) {
    const int c0 = 4 * c4;
    f32x4 v = *(const f32x4*)(si + c0);
    if (i_fresh && raw_out) *(f32x4*)(raw_out + pi * a.src_ld + c0) = v;      // the ring write of the fused call
    if (c0 + 3 >= spcol && c0 < rcol) {                   // the piece holds s' columns: those come from row m
      const f32x4 w = *(const f32x4*)(sm + c0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e >= spcol && c0 + e < rcol) v[e] = w[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c0 + e == rcol) v[e] = Gf;
      if (c0 + e == rcol + 1) v[e] = dval;
    }
    *(f32x4*)(di + c0) = v;
  }
  if (g == 0) {
    if (a.steps) a.steps[RING ? pi : i] = (unsigned char)(mo + 1);
    if (RING && i_fresh && raw_out) ends[pi] = (unsigned char)(newest_end != 0);
  }
}

// Both kernels are templates on what their call carries, instantiated where iqlhip.hip launches them — at its end: the
// compiler emits such instantiations behind every kernel defined before them, so the existing kernels keep their order.
// Rows [row0, row0 + n) of src -> the same rows of dst; ep_last (TABLE) and steps are indexed from 0 in the range.
template <bool TABLE>
__global__ __launch_bounds__(256) void iql_nstep_build_kernel(NstepArgs a, long long row0, long long n,
                                                              const long long* __restrict__ ep_last) {
  const long long rounds = (n + NS_ROWS_PER_BLOCK - 1) / NS_ROWS_PER_BLOCK;
  for (long long b = blockIdx.x; b < rounds; b += gridDim.x) {          // (uniform trip count per block)
    const long long i = b * NS_ROWS_PER_BLOCK + (threadIdx.x / NS_LANES);
    ns_row<false>(a, row0, 0, n, i < n ? i : n - 1, i < n, TABLE ? ep_last : nullptr, nullptr, nullptr, 0, nullptr);
  }
}

// The `todo` newest rows of a ring of n rows whose newest sits at position `newest` (the oldest at
// (newest - (n - 1)) mod cap): the only rows whose chains can reach the newest row.  gridDim.x * 16 >= todo.
// FUSED: the newest row comes from newest_row / newest_end and is stored into raw_out / ends (iqlhip_online_step_nstep).
template <bool FUSED>
__global__ __launch_bounds__(256) void iql_nstep_ring_kernel(NstepArgs a, long long cap, long long n, long long newest,
                                                             int todo, unsigned char* ends,
                                                             const float* __restrict__ newest_row, int newest_end,
                                                             float* raw_out) {
  long long base = newest - (n - 1);
  if (base < 0) base += cap;
  const int t = (int)blockIdx.x * NS_ROWS_PER_BLOCK + (int)(threadIdx.x / NS_LANES);
  ns_row<true>(a, base, cap, n, t < todo ? n - todo + t : n - 1, t < todo, nullptr, ends, FUSED ? newest_row : nullptr,
               FUSED ? newest_end : 0, FUSED ? raw_out : nullptr);
}

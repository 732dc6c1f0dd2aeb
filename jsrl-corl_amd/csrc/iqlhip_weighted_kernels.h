// iqlhip_weighted_kernels.h — weighted replay sampling (include/iqlhip.h "weighted replay sampling").
// Included by iqlhip.hip behind every other kernel of the library (the existing kernels keep their places in the code
// object); needs iqlhip_kernels.h (philox4x32_10, ChunkHdr, call_setup_head, dropmask_words, f32x4).
//
// The distribution is defined in integers.  q[i] = floor(w[i] * 2^(38 - e)), e = floor(log2(max w)), taken from the
// fp32 bit pattern by shifts; cum[i] = q[0] + ... + q[i] (uint64); a draw maps its 64 random bits r to
// t = mulhi64(r, cum[n - 1]) and returns the smallest i with cum[i] > t.  Every step is exact, so the table and the
// indices do not depend on how the scan is split into passes or on any floating-point mode.
//
// The table is ONE device allocation: level 0 = cum[0..n), level l + 1 = every 64th entry of level l
// (L[k] = below[min(64 k + 63, size - 1)]), up to a level of <= 64 entries; each level starts on a multiple of 64
// entries, so a node — 64 consecutive separators — is one aligned 512-byte read.
//
// An UPDATABLE table (WTab::local) has the same geometry and node-local contents — see "updatable tables" below: the
// descent then subtracts the chosen child's left neighbour from t at every level and returns the same index.
#pragma once

#define WT_MAX_LEVELS 4                 // n <= 2^24: 2^24, 2^18, 2^12, 64
#define WT_SCAN_ITEMS 16                // entries per thread of a scan block
#define WT_SCAN_TILE (256 * WT_SCAN_ITEMS)

// (WTab — what a kernel needs of a table — is defined next to IdleWork, which holds one: iqlhip_kernels.h)

// ---- building the table ----------------------------------------------------------------------------------------------
// out[0]: the largest bit pattern among the finite, non-negative weights (their order is the order of their bits);
// out[1]: bit 0 = some weight is NaN or infinite, bit 1 = some weight is negative (-0.0 counts as zero).
__global__ __launch_bounds__(256) void iql_wt_validate_kernel(const float* __restrict__ w, long long n, unsigned* out) {
  unsigned mx = 0u, bad = 0u;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const unsigned b = __float_as_uint(w[i]);
    if ((b & 0x7F800000u) == 0x7F800000u) bad |= 1u;
    else if ((b >> 31) && (b << 1)) bad |= 2u;
    else mx = max(mx, b & 0x7FFFFFFFu);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    bad |= (unsigned)__shfl_xor((int)bad, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (mx) atomicMax(out, mx);
    if (bad) atomicOr(out + 1, bad);
  }
}

// q of one weight: its significand shifted by (its exponent + sh0), sh0 = 38 - e.  (No weight exceeds the largest one,
// so a left shift never loses bits: q < 2^39.)
__device__ __forceinline__ unsigned long long wt_quantise(float w, int sh0) {
  const unsigned b = __float_as_uint(w) & 0x7FFFFFFFu;
  const unsigned ex = b >> 23;
  const unsigned long long m = ex ? (unsigned long long)((b & 0x7FFFFFu) | 0x800000u) : (unsigned long long)(b & 0x7FFFFFu);
  const int s = (ex ? (int)ex - 150 : -149) + sh0;
  if (s >= 0) return m << min(s, 39);
  return (s > -24) ? (m >> (-s)) : 0ull;
}

// Inclusive scan of one value per thread over the block's 256 threads (s_wave: 4 words of LDS).
__device__ __forceinline__ unsigned long long wt_block_scan(unsigned long long v, unsigned long long* s_wave,
                                                            unsigned long long* block_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  unsigned long long base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long t = s_wave[k];
    if (k < wave) base += t;
    tot += t;
  }
  __syncthreads();
  *block_total = tot;
  return v + base;
}

// Pass 1: bsum[b] = the sum of q over tile b (WT_SCAN_TILE weights).
__global__ __launch_bounds__(256) void iql_wt_tile_sums_kernel(const float* __restrict__ w, long long n, int sh0,
                                                               unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long s_wave[4];
  const long long i0 = (long long)blockIdx.x * WT_SCAN_TILE + (long long)threadIdx.x * WT_SCAN_ITEMS;
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < WT_SCAN_ITEMS; ++k)
    if (i0 + k < n) v += wt_quantise(w[i0 + k], sh0);
  unsigned long long tot;
  (void)wt_block_scan(v, s_wave, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// Pass 2 (one block): bsum -> its exclusive scan, in place; nb <= WT_SCAN_TILE tiles (n <= 2^24).
__global__ __launch_bounds__(256) void iql_wt_scan_sums_kernel(unsigned long long* bsum, int nb) {
  __shared__ unsigned long long s_wave[4];
  const int i0 = (int)threadIdx.x * WT_SCAN_ITEMS;
  unsigned long long x[WT_SCAN_ITEMS], v = 0;
#pragma unroll
  for (int k = 0; k < WT_SCAN_ITEMS; ++k) {
    x[k] = (i0 + k < nb) ? bsum[i0 + k] : 0ull;
    v += x[k];
  }
  unsigned long long tot;
  unsigned long long run = wt_block_scan(v, s_wave, &tot) - v;      // exclusive prefix of this thread's first entry
#pragma unroll
  for (int k = 0; k < WT_SCAN_ITEMS; ++k) {
    if (i0 + k < nb) bsum[i0 + k] = run;
    run += x[k];
  }
}

// Pass 3: cum[i] = (tiles before this one) + the inclusive scan inside the tile.
__global__ __launch_bounds__(256) void iql_wt_tile_scan_kernel(const float* __restrict__ w, long long n, int sh0,
                                                               const unsigned long long* __restrict__ bsum,
                                                               unsigned long long* __restrict__ cum) {
  __shared__ unsigned long long s_wave[4];
  const long long i0 = (long long)blockIdx.x * WT_SCAN_TILE + (long long)threadIdx.x * WT_SCAN_ITEMS;
  unsigned long long x[WT_SCAN_ITEMS], v = 0;
#pragma unroll
  for (int k = 0; k < WT_SCAN_ITEMS; ++k) {
    x[k] = (i0 + k < n) ? wt_quantise(w[i0 + k], sh0) : 0ull;
    v += x[k];
  }
  unsigned long long tot;
  unsigned long long run = wt_block_scan(v, s_wave, &tot) - v + bsum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < WT_SCAN_ITEMS; ++k) {
    run += x[k];
    if (i0 + k < n) cum[i0 + k] = run;
  }
}

// A search level from the one below: up[k] = below[min(64 k + 63, size_below - 1)], k < size_up.
__global__ __launch_bounds__(256) void iql_wt_level_kernel(const unsigned long long* __restrict__ below, unsigned size_below,
                                                           unsigned long long* __restrict__ up, unsigned size_up) {
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  if (k < size_up) up[k] = below[min(64u * k + 63u, size_below - 1u)];
}

// ---- updatable tables (iqlhip_weights_build_updatable / iqlhip_weights_update; DESIGN.md 6i "updatable tables") -------
// The same geometry, other contents: a node holds the inclusive prefix sums of its OWN 64 children's subtree totals
// (level 0: of its 64 rows' q), so a changed q[i] touches one node per level — the entries at and behind the child's
// position — and nothing else.  A node's total is its last entry; the top node's entries are global prefixes.

// Inclusive scan over the 64 lanes of a wave.
__device__ __forceinline__ unsigned long long wt_wave_scan(unsigned long long v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

// Level 0, one wave per node: tab[64 k + l] = q[64 k] + ... + q[64 k + l]; rows n_w .. cap weigh nothing.
__global__ __launch_bounds__(256) void iql_wt_local_leaves_kernel(const float* __restrict__ w, long long n_w, unsigned cap,
                                                                  int sh0, unsigned long long* __restrict__ tab) {
  const unsigned i = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u + (threadIdx.x & 63u);
  const unsigned long long v = wt_wave_scan(((long long)i < n_w) ? wt_quantise(w[i], sh0) : 0ull);
  if (i < cap) tab[i] = v;
}

// A level from the one below, one wave per node: up[64 k + c] = the totals of the node's children 0 .. c, the total of
// child node j of `below` being its last entry, below[min(64 j + 63, size_below - 1)].
__global__ __launch_bounds__(256) void iql_wt_local_level_kernel(const unsigned long long* __restrict__ below,
                                                                 unsigned size_below, unsigned long long* __restrict__ up,
                                                                 unsigned size_up) {
  const unsigned k = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u + (threadIdx.x & 63u);
  const unsigned long long v = wt_wave_scan((k < size_up) ? below[min(64u * k + 63u, size_below - 1u)] : 0ull);
  if (k < size_up) up[k] = v;
}

#define WT_Q_SATURATED ((1ull << 39) - 1ull)
#define WT_FLAG_NONFINITE 1u
#define WT_FLAG_NEGATIVE 2u
#define WT_FLAG_INDEX 4u

// What an updatable table's kernels need beyond WTab: the fixed scale and the bookkeeping.
struct WUpd {
  unsigned long long* tab;
  unsigned* stamp;                        // [n] 0, or (position of the entry that sets this row in the running update) + 1
  unsigned* flags;                        // the sticky flag word
  unsigned n;
  int levels;
  int sh0;                                // 38 - e, fixed when the table was built
  unsigned sat_bits;                      // the bit pattern of 2^(e + 1): a weight at or above it saturates
};

// Why entry (i, w) of an update is skipped (0: it is applied).
__device__ __forceinline__ unsigned wt_update_bad(long long i, float w, long long bound) {
  const unsigned b = __float_as_uint(w);
  unsigned bad = 0u;
  if ((b & 0x7F800000u) == 0x7F800000u) bad |= WT_FLAG_NONFINITE;
  else if ((b >> 31) && (b << 1)) bad |= WT_FLAG_NEGATIVE;
  if (i < 0 || i >= bound) bad |= WT_FLAG_INDEX;
  return bad;
}

// The three launches of an update take their weights from a SOURCE, a compile-time switch: WtVec — entry j's weight is
// w[j] (iqlhip_weights_update) — or WtTd (iqlhip_prio_kernels.h) — it is td_priority of entry j's TD errors, formed on the
// fly (iqlhip_weights_update_td, the prioritised chunk graphs).  The kernels below are the WtVec instantiations.
// (The bodies' pointer parameters carry no __restrict__ — the kernels' own do: with it on both, the compiler hoists the
//  kernel-argument loads of the WtVec kernels, which are to keep the code they had as plain kernels.)
struct WtVec {
  const float* __restrict__ w;
  __device__ __forceinline__ float operator()(unsigned j) const { return w[j]; }
};

// Update, launch 1: the last valid entry of every row wins (stamp[i] = max over its entries of j + 1); bad entries
// only leave their flag bits.
template <class WS>
__device__ __forceinline__ void wt_update_stamp(const long long* idx, const WS& w, unsigned m, long long bound,
                                                const WUpd& t) {
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  unsigned bad = 0u;
  if (j < m) {
    const long long i = idx[j];
    bad = wt_update_bad(i, w(j), bound);
    if (!bad) atomicMax(t.stamp + i, j + 1u);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad |= (unsigned)__shfl_xor((int)bad, o);
  if ((threadIdx.x & 63) == 0 && bad) atomicOr(t.flags, bad);
}
__global__ __launch_bounds__(256) void iql_wt_update_stamp_kernel(const long long* __restrict__ idx, const float* __restrict__ w,
                                                                  unsigned m, long long bound, WUpd t) {
  wt_update_stamp(idx, WtVec{w}, m, bound, t);
}

// Launch 2: delta[j] = q_new - q_old (two's complement) of every winner, q_old read back from its level-0 node —
// nothing writes the tree in this launch.  Entries that lost or are skipped get 0.
// TRACK (a tracking table, iqlhip_weights_build_tracking): the largest q_new among the launch's winners is also raised
// into the table's maximum word — a maximum over the wave first, then one 64-bit atomic maximum per wave that has a
// winner.  Entries that lost or are skipped raise nothing.  TRACK = false is the code the kernels always had.
template <class WS, bool TRACK = false>
__device__ __forceinline__ void wt_update_delta(const long long* idx, const WS& w, unsigned m, long long bound,
                                                const WUpd& t, unsigned long long* delta, unsigned long long* q_max = nullptr) {
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  if (!TRACK && j >= m) return;
  unsigned long long won = 0ull;
  if (j < m) {
    const long long i = idx[j];
    const float wj = w(j);
    unsigned long long d = 0ull;
    if (!wt_update_bad(i, wj, bound) && t.stamp[i] == j + 1u) {
      const unsigned long long upto = t.tab[i], before = (i & 63) ? t.tab[i - 1] : 0ull;
      const unsigned long long q_new =
          ((__float_as_uint(wj) & 0x7FFFFFFFu) >= t.sat_bits) ? WT_Q_SATURATED : wt_quantise(wj, t.sh0);
      d = q_new - (upto - before);
      won = q_new;
    }
    delta[j] = d;
  }
  if (TRACK) {      // (every lane of the wave is here: no lane has returned)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long u = __shfl_xor(won, o);
      won = u > won ? u : won;
    }
    if ((threadIdx.x & 63) == 0 && won) atomicMax(q_max, won);
  }
}
__global__ __launch_bounds__(256) void iql_wt_update_delta_kernel(const long long* __restrict__ idx, const float* __restrict__ w,
                                                                  unsigned m, long long bound, WUpd t,
                                                                  unsigned long long* __restrict__ delta) {
  wt_update_delta(idx, WtVec{w}, m, bound, t, delta);
}

// Launch 3, one wave per entry: a winner adds its delta to the entries at and behind its position in its node of every
// level (waves of different rows meet in the upper nodes: 64-bit atomic adds, which commute), and resets its stamp.
template <class WS>
__device__ __forceinline__ void wt_update_apply(const long long* idx, const WS& w, unsigned m, long long bound,
                                                const WUpd& t, const unsigned long long* delta) {
  const unsigned j = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  const unsigned lane = threadIdx.x & 63u;
  if (j >= m) return;
  const long long i = idx[j];
  if (wt_update_bad(i, w(j), bound) || t.stamp[i] != j + 1u) return;
  const unsigned long long d = delta[j];
  if (d) {
    unsigned size = t.n, off = 0u, at = (unsigned)i;
#pragma unroll
    for (int l = 0; l < WT_MAX_LEVELS; ++l) {
      if (l < t.levels) {
        const unsigned first = at & ~63u, width = min(64u, size - first);
        if (lane >= (at & 63u) && lane < width) atomicAdd(t.tab + off + first + lane, d);
      }
      off += (size + 63u) & ~63u;
      size = (size + 63u) >> 6;
      at >>= 6;
    }
  }
  if (lane == 0) t.stamp[i] = 0u;
}
__global__ __launch_bounds__(256) void iql_wt_update_apply_kernel(const long long* __restrict__ idx, const float* __restrict__ w,
                                                                  unsigned m, long long bound, WUpd t,
                                                                  const unsigned long long* __restrict__ delta) {
  wt_update_apply(idx, WtVec{w}, m, bound, t, delta);
}

// Leaf values back from the tree (iqlhip_weights_state): q[i] = tab[i] - tab[i - 1], or tab[i] where a node begins
// (local) or at i == 0 (a static table's global cum).
__global__ __launch_bounds__(256) void iql_wt_leaves_kernel(const unsigned long long* __restrict__ tab, unsigned n, int local,
                                                            unsigned long long* __restrict__ q) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) q[i] = tab[i] - (((local ? (i & 63u) : i) != 0u) ? tab[i - 1] : 0ull);
}

// ---- the draw --------------------------------------------------------------------------------------------------------
// The 64 random bits of index j of a call: draw_index's (iqlhip_kernels.h) — same counter, same tag, same word pair.
__device__ __forceinline__ unsigned long long wt_draw_bits(unsigned long long seed, unsigned long long ctr0, unsigned long long j) {
  const unsigned long long ctr = ctr0 + (j >> 1);
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0x49514C48u /* "IQLH" */, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (j & 1ull) ? (((unsigned long long)c[3] << 32) | c[2]) : (((unsigned long long)c[1] << 32) | c[0]);
}

// U indices resolved by ONE wave, all of its lanes calling with the same arguments: a 64-ary descent from the top level.
// At each level lane l reads separator l of the current node (one coalesced 512-byte read; lanes past the node's width
// count as "greater"), and the child is the number of separators <= t — the population count of a 64-bit ballot, clamped
// to the node's width so that no table content can lead outside the table.  The top node's last separator is
// cum[n - 1], the total t is scaled by.  The U descents are independent: their reads of a level are in flight together.
template <int U>
__device__ __forceinline__ void draw_index_weighted(const WTab& wt, unsigned long long seed, unsigned long long ctr0,
                                                    const unsigned long long (&j)[U], long long (&out)[U]) {
  const unsigned lane = threadIdx.x & 63u;
  unsigned size[WT_MAX_LEVELS], off[WT_MAX_LEVELS];
  {
    unsigned s = wt.n, o = 0;
#pragma unroll
    for (int l = 0; l < WT_MAX_LEVELS; ++l) {
      size[l] = s; off[l] = o;
      o += (s + 63u) & ~63u;
      s = (s + 63u) >> 6;
    }
  }
  unsigned long long r[U], t[U];
  unsigned node[U];
#pragma unroll
  for (int u = 0; u < U; ++u) { r[u] = wt_draw_bits(seed, ctr0, j[u]); node[u] = 0u; t[u] = 0ull; }
#pragma unroll
  for (int l = WT_MAX_LEVELS - 1; l >= 0; --l) {
    if (l == 0 || size[l > 0 ? l - 1 : 0] > 64u) {      // l < wt.levels, told from the sizes the descent holds anyway
      unsigned long long sep[U];
      unsigned width[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const unsigned first = 64u * node[u];
        width[u] = min(64u, size[l] - first);
        sep[u] = (lane < width[u]) ? wt.tab[off[l] + first + lane] : ~0ull;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (size[l] <= 64u) {           // the top level: l == wt.levels - 1
          const unsigned long long total = __shfl(sep[u], (int)width[u] - 1);
          t[u] = __umul64hi(r[u], total);
        }
        const unsigned child = min((unsigned)__popcll(__ballot(lane < width[u] && sep[u] <= t[u])), width[u] - 1u);
        node[u] = 64u * node[u] + child;
        if (wt.local) {                 // (uniform over the wave) node-local prefixes: t becomes relative to the child
          const unsigned long long before = __shfl(sep[u], (int)max(child, 1u) - 1);
          t[u] -= child ? before : 0ull;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) out[u] = (long long)node[u];
}

// idx[j] = weighted index j of the stream (seed, offset), j < n_idx: one wave per index, two in flight per wave.
__global__ __launch_bounds__(256) void iql_draw_indices_weighted_kernel(long long* idx, long long n_idx, WTab wt,
                                                                        unsigned long long seed, unsigned long long offset) {
  const long long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  const long long n_waves = (long long)gridDim.x * 4;
  for (long long j0 = wave; j0 < n_idx; j0 += 2 * n_waves) {
    const long long j1 = j0 + n_waves;
    const unsigned long long j[2] = {(unsigned long long)j0, (unsigned long long)(j1 < n_idx ? j1 : j0)};
    long long i[2];
    draw_index_weighted<2>(wt, seed, offset, j, i);
    if ((threadIdx.x & 63) == 0) {
      idx[j0] = i[0];
      if (j1 < n_idx) idx[j1] = i[1];
    }
  }
}

// rows[weighted draw(j0 + r)] -> xb[r], r < n: gather_rows_drawn with the index of a row resolved by the wave that then
// copies it — the index never leaves the wave's registers (no LDS, no scratch, no barrier).  wave / n_waves: this
// wave's number and the count of waves sharing the work; two rows per pass, their descents in flight together.
__device__ __forceinline__ void gather_rows_drawn_weighted(const float* rows, long long ld, float* xb, int n, const WTab& wt,
                                                           unsigned long long seed, unsigned long long ctr0,
                                                           unsigned long long j0, int wave, int n_waves) {
  const int q = (int)(ld >> 2);
  const int lane = (int)(threadIdx.x & 63);
  for (int r0 = wave; r0 < n; r0 += 2 * n_waves) {
    const int r1 = r0 + n_waves;
    const bool two = r1 < n;
    const unsigned long long j[2] = {j0 + (unsigned long long)r0, j0 + (unsigned long long)(two ? r1 : r0)};
    long long i[2];
    draw_index_weighted<2>(wt, seed, ctr0, j, i);
    for (int c4 = lane; c4 < q; c4 += 64) {
      const f32x4 a = *(const f32x4*)(rows + i[0] * ld + 4 * c4);
      f32x4 b = a;
      if (two) b = *(const f32x4*)(rows + i[1] * ld + 4 * c4);
      *(f32x4*)(xb + (long long)r0 * ld + 4 * c4) = a;
      if (two) *(f32x4*)(xb + (long long)r1 * ld + 4 * c4) = b;
    }
  }
}

// The idle work of a weighted chunk's forward (idle_block_work<2>): the next step's rows, drawn by weight.
__device__ __forceinline__ void idle_gather_weighted(const IdleWork& w, unsigned long long seed, unsigned long long ctr0,
                                                     unsigned long long j0, int blk, int nblk) {
  const WTab wt = w.wt;
  const int wave = __builtin_amdgcn_readfirstlane(blk * 4 + (int)(threadIdx.x >> 6));
  gather_rows_drawn_weighted(w.rows, w.ld, w.xb_dst, w.n, wt, seed, ctr0, j0, wave, nblk * 4);
}

// First launch of an iqlhip_train_steps_weighted call: iql_call_setup_kernel with step 0's rows drawn by weight
// (B == 0: the previous weighted call on this table left them staged).
__global__ __launch_bounds__(256) void iql_call_setup_weighted_kernel(unsigned long long* hdr, ChunkHdr h,
                                                                      iqlhip_step_scalars* sched_call,
                                                                      const iqlhip_step_scalars* sched_src, int n_steps,
                                                                      const float* rows, long long ld, float* xb, int B,
                                                                      unsigned* drop_dst, int drop_words, unsigned drop_thresh,
                                                                      unsigned* arrivals, unsigned long long* ack,
                                                                      unsigned long long ack_val, WTab wt) {
  call_setup_head(hdr, h, sched_call, sched_src, n_steps, arrivals, ack, ack_val);
  if (B > 0)
    gather_rows_drawn_weighted(rows, ld, xb, B, wt, h.w[HDR_SEED], h.w[HDR_OFFSET], h.w[HDR_POS],
                               __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6))), (int)gridDim.x * 4);
  if (drop_dst)
    dropmask_words(drop_dst, drop_words, drop_thresh, h.w[HDR_DROP_SEED], h.w[HDR_DROP_STEP],
                   ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// The training forward of a weighted chunk: iql_fwd_kernel's body a third time, the idle blocks drawing the next step's
// rows by weight (idle_block_work<2>).  A kernel of its own, as iql_fwd_mixed_kernel is: plain calls' forward stays as it is.
template <bool BF16, bool W0DMA, bool MULTI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_fwd_weighted_kernel(StepParams p) {
  constexpr bool ONE = false, ROW_EXIT = false;
  constexpr int MIXED_IDLE = 2;
  FWD_NOT_EARLY();
#include "iqlhip_fwd_body.inc"
}

// ---- trainer groups (iqlhip_group_train_steps_weighted; DESIGN.md 6i "trainer groups") --------------------------------
// (GroupWtRec — one record per member, an array of its own next to the GroupRecs, as GroupDropRec is — is defined with
//  the group records: iqlhip_kernels.h.  GroupRec itself is unchanged.)
// One member's rows of step s: by its table (one wave resolves an index and copies that row; `wave` is uniform across
// the wave, so the descent's addresses stay scalar), or — no table — iql_gather_group_kernel's uniform draw with its
// arguments.  The branch is uniform per block: a block serves one member.
__device__ __forceinline__ void group_gather_weighted(const GroupRec& r, const GroupWtRec& w, int s) {
  const unsigned long long j0 = (unsigned long long)s * (unsigned long long)r.B;
  if (w.wt.tab) {
    const WTab wt = w.wt;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    gather_rows_drawn_weighted(r.rows, r.ld, r.xb, r.B, wt, r.seed, r.offset, j0, wave, (int)gridDim.x * 4);
  } else {
    gather_rows_drawn(r.rows, r.ld, r.xb, r.B, r.seed, r.offset, j0, (unsigned long long)r.size,
                      (int)blockIdx.x * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
  }
}

// iql_gather_group_kernel with member blockIdx.y's rows drawn by wts[blockIdx.y] (a null table: uniformly).
__global__ __launch_bounds__(256) void iql_gather_weighted_group_kernel(const GroupRec* __restrict__ recs,
                                                                        const GroupWtRec* __restrict__ wts, int step) {
  const GroupRec& r = recs[blockIdx.y];
  const int s = min(max(step, 0), r.n_steps - 1);
  group_gather_weighted(r, wts[blockIdx.y], s);
}

// ... plus the step's keep-bit words of the members that draw some, from the far end of the grid
// (iql_gather_drop_group_kernel's split).  Launched only when some member of the call draws keep-bits.
__global__ __launch_bounds__(256) void iql_gather_weighted_drop_group_kernel(const GroupRec* __restrict__ recs,
                                                                             const GroupWtRec* __restrict__ wts,
                                                                             const GroupDropRec* __restrict__ drops, int step) {
  const GroupRec& r = recs[blockIdx.y];
  const int s = min(max(step, 0), r.n_steps - 1);
  group_gather_weighted(r, wts[blockIdx.y], s);
  const GroupDropRec& d = drops[blockIdx.y];
  if (d.active)
    group_drop_words(d, d.step0 + (unsigned long long)s, ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x,
                     (int)gridDim.x * 256);
}

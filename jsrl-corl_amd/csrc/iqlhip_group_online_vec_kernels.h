// iqlhip_group_online_vec_kernels.h — the buffer work of the trainer groups' vector-environment online call
// (iqlhip_group_online_step_vec; include/iqlhip.h "group vector-environment online step").
// Included by iqlhip.hip behind every other kernel: what it adds lies at the end of the code object and everything that
// existed keeps its place there.
#pragma once

// One record per member (grid.y): what iql_online_vec_gather_kernel takes as arguments, plus the act states.
struct GroupVecRec {
  float* rows;                        // the member's ring (packed rows, stride ld, `capacity` rows)
  const float* rows_pin;              // its n_new new transitions [n_new][ld] (pinned, host-mapped)
  const long long* idx_pin;           // its n = U * B drawn indices (pinned, host-mapped), the steps' one behind the other
  float* xb;                          // its slice of the group's staging block [U][B][ld]
  const float* act_pin;               // its act states [act_rows][S] (pinned, host-mapped) or NULL: no action requested
  float* xb_act;                      // its inference staging
  long long ld, capacity, pointer;
  int n_new, n, act_rows, S;
};

// iql_online_vec_gather_kernel per member: the n_new ring writes at (pointer + j) mod capacity, the gather of the n drawn
// rows into the member's staging slice, and the packing of its act_rows act states into xb_act (iql_pack_states_kernel's
// rows: the state in the first S columns, zeros behind).  The solo kernel's hazard rule holds per member: a drawn index i
// with (i - pointer) mod capacity < n_new is read from rows_pin, never from the ring — the write of that row belongs to
// another block (or a later wave) and may not have landed.  Copies are 16 bytes wide; element e = 256 * block + thread is
// float4 column e % (ld / 4) of row e / (ld / 4), of the new rows, of the act rows and of the batch alike; a block's
// indices (at most 256 / (ld / 4) + 2 rows) are staged in LDS first.  The grid is sized for the largest member: a block
// past a member's own counts reads no index and stores nothing.
// Preconditions (checked by the host, per member): 0 <= pointer < capacity, 1 <= n_new <= capacity, every index in
// [0, capacity), ld a multiple of 4 and >= 8, rows / rows_pin / xb / xb_act 16-byte aligned, n * (ld / 4) < 2^31.
__device__ __forceinline__ void online_vec_gather_member(const GroupVecRec& g) {
  __shared__ long long s_idx[260];
  float* rows = g.rows;
  const float* rows_pin = g.rows_pin;
  const long long ld = g.ld, capacity = g.capacity, pointer = g.pointer;
  const int n = g.n, n_new = g.n_new;
  const int q = (int)(ld >> 2);
  const int e0 = (int)blockIdx.x * 256;
  const int e = e0 + (int)threadIdx.x;
  const int r_first = e0 / q;
  if (e0 < n * q) {
    const int r_last = min((e0 + 255) / q, n - 1);
    if ((int)threadIdx.x <= r_last - r_first) s_idx[threadIdx.x] = g.idx_pin[r_first + threadIdx.x];
  }
  if (e < n_new * q) {
    const int j = e / q, c4 = e - j * q;
    long long dst = pointer + j;
    if (dst >= capacity) dst -= capacity;
    *(f32x4*)(rows + dst * ld + 4 * c4) = *(const f32x4*)(rows_pin + (long long)j * ld + 4 * c4);
  }
  if (g.act_pin && e < g.act_rows * q) {
    const int j = e / q, c4 = e - j * q;
    const float* s = g.act_pin + (long long)j * g.S;
    f32x4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = (4 * c4 + t < g.S) ? s[4 * c4 + t] : 0.f;
    *(f32x4*)(g.xb_act + (long long)j * ld + 4 * c4) = v;
  }
  __syncthreads();
  if (e < n * q) {
    const int r = e / q, c4 = e - r * q;
    const long long i = s_idx[r - r_first];
    long long d = i - pointer;
    if (d < 0) d += capacity;
    const float* src = (d < (long long)n_new) ? rows_pin + d * ld : rows + i * ld;
    *(f32x4*)(g.xb + (long long)r * ld + 4 * c4) = *(const f32x4*)(src + 4 * c4);
  }
}
__global__ __launch_bounds__(256) void iql_online_vec_gather_group_kernel(const GroupVecRec* __restrict__ recs) {
  online_vec_gather_member(recs[blockIdx.y]);
}
// ... plus the keep-bits of the act forwards that run with dropout (drops[member]; launched instead of the kernel above
// only when some requesting member's inference rate is > 0): act_rows rows' words, from the far end of the grid
// (iql_online_gather_drop_group_kernel's split).
__global__ __launch_bounds__(256) void iql_online_vec_gather_drop_group_kernel(const GroupVecRec* __restrict__ recs,
                                                                               const ActDropRec* __restrict__ drops) {
  online_vec_gather_member(recs[blockIdx.y]);
  const ActDropRec& d = drops[blockIdx.y];
  if (d.active)
    act_drop_words(d, ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// iqlhip_online_vec_kernels.h — the buffer work of the vector-environment online call (iqlhip_online_step_vec) and of
// the multi-row ring write (iqlhip_rows_write_ring; include/iqlhip.h "vector-environment online step").
// Included by iqlhip.hip behind every other kernel: what it adds lies at the end of the code object and everything that
// existed keeps its place there.
#pragma once

// One launch: the n_new transitions rows_host[j] (pinned, host-mapped, n_new x ld floats, j in row order) are stored at
// ring rows (pointer + j) mod capacity, and the n rows rows[idx_host[r]] (indices in pinned, host-mapped memory, as
// np.random.randint drew them over the size after the inserts) are gathered into xb[r] — n = U * B rows, the batches of
// the call's U steps one behind the other.  A drawn index i with (i - pointer) mod capacity < n_new names one of the new
// rows: it is read from rows_host itself, because the ring write of that row belongs to another block (or a later wave)
// and may not have happened yet — iql_online_gather_kernel's rule for its one row.  No other ring row is written, so
// every other read sees what the launches before this one left.  n = 0 (idx_host and xb unused): the ring write alone.
// Copies are 16 bytes wide; element e = 256 * block + thread is float4 column e % (ld / 4) of row e / (ld / 4), of the new
// rows and of the batch alike; a block's indices (at most 256 / (ld / 4) + 2 rows) are staged in LDS first.
// Preconditions (checked by the host): 0 <= pointer < capacity, 1 <= n_new <= capacity, every index in [0, capacity),
// ld a multiple of 4 and >= 8, rows / rows_host / xb 16-byte aligned, n * (ld / 4) < 2^31.
__global__ __launch_bounds__(256) void iql_online_vec_gather_kernel(float* rows, long long ld, long long capacity,
                                                                    long long pointer, const float* rows_host, int n_new,
                                                                    const long long* idx_host, float* xb, int n) {
  __shared__ long long s_idx[260];
  const int q = (int)(ld >> 2);
  const int e0 = (int)blockIdx.x * 256;
  const int e = e0 + (int)threadIdx.x;
  const int r_first = e0 / q;
  if (e0 < n * q) {
    const int r_last = min((e0 + 255) / q, n - 1);
    if ((int)threadIdx.x <= r_last - r_first) s_idx[threadIdx.x] = idx_host[r_first + threadIdx.x];
  }
  if (e < n_new * q) {
    const int j = e / q, c4 = e - j * q;
    long long dst = pointer + j;
    if (dst >= capacity) dst -= capacity;
    *(f32x4*)(rows + dst * ld + 4 * c4) = *(const f32x4*)(rows_host + (long long)j * ld + 4 * c4);
  }
  __syncthreads();
  if (e < n * q) {
    const int r = e / q, c4 = e - r * q;
    const long long i = s_idx[r - r_first];
    long long d = i - pointer;
    if (d < 0) d += capacity;
    const float* src = (d < (long long)n_new) ? rows_host + d * ld : rows + i * ld;
    *(f32x4*)(xb + (long long)r * ld + 4 * c4) = *(const f32x4*)(src + 4 * c4);
  }
}

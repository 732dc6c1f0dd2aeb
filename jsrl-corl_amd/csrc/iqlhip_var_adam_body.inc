// iqlhip_var_adam_body.inc — the body of iql_var_adam_kernel and iql_var_adam_group_kernel (iqlhip_variance_kernels.h).
// In scope: float *pw, *m, *v; const float* gr; int n, i (the word); float step_neg, bc2, omb1, b2, omb2, eps.
  if (i >= n) return;
  const float gk = gr[i];
  const float mk = fmaf(omb1, gk - m[i], m[i]);
  const float vk = fmaf(omb2 * gk, gk, v[i] * b2);
  const float denom = sqrtf(vk) / bc2 + eps;
  m[i] = mk;
  v[i] = vk;
  pw[i] = fmaf(step_neg, mk / denom, pw[i]);

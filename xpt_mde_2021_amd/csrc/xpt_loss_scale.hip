// xpt_loss_scale.hip -- the on-device state machine of dynamic loss scaling (half-precision build, row a14b).
// Replaces the DynamicLossScale of tf.keras.mixed_precision LossScaleOptimizer (TF 2.4): after the flat gradient is final
// (L2 terms added, all-reduced), ONE launch raises found_inf when any element is +-inf or NaN; the optimizer launch
// (xpt_adam_step_dyn / xpt_sgd_step_dyn, xpt_optim.hip) skips the update on it; ONE single-workgroup launch then halves or
// grows the scale and clears the flag.  Nothing here needs the host: the steps replay from a hipGraph as they are.
#include "xpt_common.h"

namespace {

// exponent field all ones: +-inf or NaN.  Integer test on the bits: a fast-math build cannot assume it away.
__device__ __forceinline__ unsigned xpt_nonfinite_bits(float x) {
  return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

__global__ void grad_nonfinite_kernel(const float* __restrict__ g, long long n, int* __restrict__ found) {
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  unsigned bad = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 v = g4[i];
    bad |= xpt_nonfinite_bits(v.x) | xpt_nonfinite_bits(v.y) | xpt_nonfinite_bits(v.z) | xpt_nonfinite_bits(v.w);
  }
  for (long long i = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride)
    bad |= xpt_nonfinite_bits(g[i]);
  // one device-scope atomic per workgroup that saw a non-finite value (none at all on a healthy step)
  if (__syncthreads_or((int)bad) && threadIdx.x == 0) atomicOr(found, 1);
}

__global__ void loss_scale_update_kernel(xpt_loss_scale_state* st, int growth_steps) {
  if (threadIdx.x != 0) return;
  float s = st->scale;
  int good = st->good_steps;
  if (st->found_inf) {
    s = fmaxf(0.5f * s, 1.f);
    good = 0;
    st->skipped = st->skipped + 1;
  } else if (++good >= growth_steps) {
    const float s2 = 2.f * s;
    if (!xpt_nonfinite_bits(s2)) s = s2;
    good = 0;
  }
  st->scale = s;
  st->inv_scale = 1.f / s;           // S is a power of two: exact
  st->good_steps = good;
  st->found_inf = 0;
}

}  // namespace

extern "C" int xpt_grad_nonfinite(const float* g, long long n, void* state, void* stream) {
  XPT_CHECK_PTR(g); XPT_CHECK_PTR(state);
  if (n <= 0) return XPT_ERR_SHAPE;
  if ((((uintptr_t)g | (uintptr_t)state) & 15) != 0) return XPT_ERR_ARG;
  long long blocks = ((n >> 2) + 255) / 256;
  if (blocks > 2048) blocks = 2048;   // as adam_kernel: 256 CUs x 8 blocks, grid-stride the rest
  if (blocks < 1) blocks = 1;
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(grad_nonfinite_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, n,
                     &static_cast<xpt_loss_scale_state*>(state)->found_inf);
  return xpt_launch_status();
}

extern "C" int xpt_loss_scale_update(void* state, int growth_steps, void* stream) {
  XPT_CHECK_PTR(state);
  if (growth_steps <= 0) return XPT_ERR_ARG;
  if (((uintptr_t)state & 15) != 0) return XPT_ERR_ARG;
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     static_cast<xpt_loss_scale_state*>(state), growth_steps);
  return xpt_launch_status();
}

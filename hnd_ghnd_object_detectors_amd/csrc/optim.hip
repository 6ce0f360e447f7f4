// hnd_optim_step_flat (include/hnd_optim.h): Adam with weight decay / AMSGrad, Adagrad and RMSprop over a flat arena.
// HBM-bound streaming passes like adam_kernel of elementwise.hip: 256 threads, grid-stride, 16 bytes per lane where every
// buffer is 16-byte aligned (decided on the host), scalar accesses for numel % 4 and for unaligned buffers.  The kind and
// its flags are template parameters: no per-element branch.  Each element is read once and stored once per buffer.
#include "common.h"

#include <math.h>

#include "hnd_optim.h"

namespace {

using hnd::f32x4;

constexpr int kMaxBlocks = 256 * 16;          // as elementwise.hip

inline int grid_for(long long work_items, int threads = 256) {
  long long b = (work_items + threads - 1) / threads;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (int)b;
}

// the launch's scalars, each rounded to fp32 once on the host
struct Scalars {
  float grad_scale, weight_decay, eps;
  float w1;          // ADAM 1 - beta1
  float beta2, w2;   // ADAM beta2 / RMSPROP alpha, and 1 - it
  float bc2_sqrt;    // ADAM sqrt(1 - beta2^step)
  float step_size;   // ADAM lr / (1 - beta1^step); ADAGRAD clr; RMSPROP lr
  float momentum;    // RMSPROP
};

// Every rounding below is spelled out -- fmaf where a product is fused into a sum, contraction off for the rest -- so the
// 16-byte body, the scalar tail and the unaligned build give one element the same bits: a tensor stepped inside the flat
// arena and stepped on its own (the per-tensor host path) ends up identical.
// torch's lerp (ATen/native/Lerp.h)
__device__ __forceinline__ float lerp_torch(float a, float b, float w) {
#pragma clang fp contract(off)
  const float d = b - a;
  return w < 0.5f ? fmaf(w, d, a) : fmaf(-d, 1.f - w, b);
}

// one element: p and the states are updated in place (registers).  F0: ADAM amsgrad / RMSPROP centered; F1: RMSPROP momentum
template <int KIND, bool F0, bool F1>
__device__ __forceinline__ void update(float& p, float gr, float& s0, float& s1, float& s2, const Scalars& k) {
#pragma clang fp contract(off)
  const float g = fmaf(k.weight_decay, p, gr * k.grad_scale);
  if constexpr (KIND == HND_OPTIM_ADAM) {
    s0 = lerp_torch(s0, g, k.w1);
    s1 = fmaf(k.w2 * g, g, s1 * k.beta2);
    float u = s1;
    if constexpr (F0) {
      s2 = fmaxf(s2, s1);
      u = s2;
    }
    const float denom = sqrtf(u) / k.bc2_sqrt + k.eps;
    p = fmaf(-k.step_size, s0 / denom, p);
  } else if constexpr (KIND == HND_OPTIM_ADAGRAD) {
    s0 = fmaf(g, g, s0);
    p = fmaf(-k.step_size, g / (sqrtf(s0) + k.eps), p);
  } else {
    s0 = fmaf(k.w2 * g, g, s0 * k.beta2);
    float avg;
    if constexpr (F0) {
      s2 = lerp_torch(s2, g, k.w2);
      avg = sqrtf(fmaf(-s2, s2, s0)) + k.eps;
    } else {
      avg = sqrtf(s0) + k.eps;
    }
    if constexpr (F1) {
      s1 = fmaf(s1, k.momentum, g / avg);
      p = fmaf(-k.step_size, s1, p);
    } else {
      p = fmaf(-k.step_size, g / avg, p);
    }
  }
}

template <int KIND, bool F0, bool F1>
struct Uses {   // which state slots the build touches
  static constexpr bool s1 = KIND == HND_OPTIM_ADAM || (KIND == HND_OPTIM_RMSPROP && F1);
  static constexpr bool s2 = (KIND == HND_OPTIM_ADAM || KIND == HND_OPTIM_RMSPROP) && F0;
};

template <int KIND, bool F0, bool F1>
__device__ __forceinline__ void update_at(float* p, const float* g, float* s0, float* s1, float* s2, long long e,
                                          const Scalars& k) {
  using U = Uses<KIND, F0, F1>;
  float pv = p[e], a = s0[e], b = 0.f, c = 0.f;
  if constexpr (U::s1) b = s1[e];
  if constexpr (U::s2) c = s2[e];
  update<KIND, F0, F1>(pv, g[e], a, b, c, k);
  p[e] = pv;
  s0[e] = a;
  if constexpr (U::s1) s1[e] = b;
  if constexpr (U::s2) s2[e] = c;
}

// VEC: whole float4s by grid-stride, then the numel % 4 last elements by the first threads of block 0; every pointer is
// 16-byte aligned.  !VEC: every element by grid-stride, 4-byte accesses.
template <int KIND, bool F0, bool F1, bool VEC>
__global__ void __launch_bounds__(256) optim_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ s0, float* __restrict__ s1,
                                                    float* __restrict__ s2, long long n, Scalars k) {
  using U = Uses<KIND, F0, F1>;
  const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    const long long n4 = n >> 2;
    for (long long e = tid; e < n4; e += stride) {
      f32x4 pv = *(const f32x4*)(p + e * 4);
      const f32x4 gv = *(const f32x4*)(g + e * 4);
      f32x4 a = *(const f32x4*)(s0 + e * 4), b = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
      if constexpr (U::s1) b = *(const f32x4*)(s1 + e * 4);
      if constexpr (U::s2) c = *(const f32x4*)(s2 + e * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float pi = pv[i], ai = a[i], bi = b[i], ci = c[i];
        update<KIND, F0, F1>(pi, gv[i], ai, bi, ci, k);
        pv[i] = pi; a[i] = ai; b[i] = bi; c[i] = ci;
      }
      *(f32x4*)(p + e * 4) = pv;
      *(f32x4*)(s0 + e * 4) = a;
      if constexpr (U::s1) *(f32x4*)(s1 + e * 4) = b;
      if constexpr (U::s2) *(f32x4*)(s2 + e * 4) = c;
    }
    const long long e = n4 * 4 + tid;      // tid < 4 only: block 0
    if (tid < (n & 3)) update_at<KIND, F0, F1>(p, g, s0, s1, s2, e, k);
  } else {
    for (long long e = tid; e < n; e += stride) update_at<KIND, F0, F1>(p, g, s0, s1, s2, e, k);
  }
}

template <int KIND, bool F0, bool F1>
void launch(const hnd_optim_desc& d, bool vec, const Scalars& k, hipStream_t s) {
  const long long n = d.numel;
  if (vec)
    hipLaunchKernelGGL((optim_kernel<KIND, F0, F1, true>), dim3(grid_for(n >> 2)), dim3(256), 0, s, d.param, d.grad,
                       d.state0, d.state1, d.state2, n, k);
  else
    hipLaunchKernelGGL((optim_kernel<KIND, F0, F1, false>), dim3(grid_for(n)), dim3(256), 0, s, d.param, d.grad, d.state0,
                       d.state1, d.state2, n, k);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int hnd_optim_abi(void) { return HND_OPTIM_ABI; }

extern "C" int hnd_optim_step_flat(const hnd_optim_desc* dp, void* stream) {
  HND_REQUIRE(dp, "hnd_optim_step_flat: null descriptor");
  const hnd_optim_desc& d = *dp;
  HND_REQUIRE(d.kind == HND_OPTIM_ADAM || d.kind == HND_OPTIM_ADAGRAD || d.kind == HND_OPTIM_RMSPROP,
              "hnd_optim_step_flat: unknown kind %d", (int)d.kind);
  const bool adam = d.kind == HND_OPTIM_ADAM, rms = d.kind == HND_OPTIM_RMSPROP;
  const bool f0 = adam ? d.amsgrad != 0 : (rms && d.centered != 0), f1 = rms && d.momentum > 0;
  const bool use1 = adam || f1, use2 = f0;
  HND_REQUIRE(d.param && d.grad, "hnd_optim_step_flat: null param or grad");
  HND_REQUIRE(d.state0 && (!use1 || d.state1) && (!use2 || d.state2),
              "hnd_optim_step_flat: a state buffer this kind / these flags use is null");
  HND_REQUIRE(d.numel > 0 && d.step >= 1, "hnd_optim_step_flat: numel %lld must be > 0 and step %lld >= 1",
              (long long)d.numel, (long long)d.step);
  const double hyper[] = {d.grad_scale, d.lr, d.weight_decay, d.eps, d.beta1, d.beta2, d.momentum, d.lr_decay};
  for (double h : hyper) HND_REQUIRE(isfinite(h), "hnd_optim_step_flat: a hyper-parameter is NaN or infinite");
  HND_REQUIRE(d.lr >= 0 && d.eps >= 0 && d.weight_decay >= 0 && d.momentum >= 0 && d.lr_decay >= 0,
              "hnd_optim_step_flat: lr, eps, weight_decay, momentum and lr_decay must be >= 0");
  if (adam)
    HND_REQUIRE(d.beta1 >= 0 && d.beta1 < 1 && d.beta2 >= 0 && d.beta2 < 1,
                "hnd_optim_step_flat: Adam betas (%g, %g) must lie in [0, 1)", d.beta1, d.beta2);
  if (rms) HND_REQUIRE(d.beta2 >= 0, "hnd_optim_step_flat: RMSprop alpha %g must be >= 0", d.beta2);
  const void* ptrs[] = {d.param, d.grad, d.state0, use1 ? d.state1 : nullptr, use2 ? d.state2 : nullptr};
  bool vec = true;
  for (const void* p : ptrs) {
    HND_REQUIRE(((uintptr_t)p & 3) == 0, "hnd_optim_step_flat: buffers must be 4-byte aligned");
    vec = vec && aligned16(p);
  }

  Scalars k = {};
  k.grad_scale = (float)d.grad_scale;
  k.weight_decay = (float)d.weight_decay;
  k.eps = (float)d.eps;
  k.beta2 = (float)d.beta2;
  k.w2 = (float)(1.0 - d.beta2);
  k.momentum = (float)d.momentum;
  if (adam) {
    k.w1 = (float)(1.0 - d.beta1);
    k.bc2_sqrt = (float)sqrt(1.0 - pow(d.beta2, (double)d.step));
    k.step_size = (float)(d.lr / (1.0 - pow(d.beta1, (double)d.step)));
  } else if (rms) {
    k.step_size = (float)d.lr;
  } else {
    k.step_size = (float)(d.lr / (1.0 + (double)(d.step - 1) * d.lr_decay));
  }
  hipStream_t s = hnd::as_stream(stream);
  if (adam) {
    if (f0) launch<HND_OPTIM_ADAM, true, false>(d, vec, k, s);
    else launch<HND_OPTIM_ADAM, false, false>(d, vec, k, s);
  } else if (rms) {
    if (f0 && f1) launch<HND_OPTIM_RMSPROP, true, true>(d, vec, k, s);
    else if (f0) launch<HND_OPTIM_RMSPROP, true, false>(d, vec, k, s);
    else if (f1) launch<HND_OPTIM_RMSPROP, false, true>(d, vec, k, s);
    else launch<HND_OPTIM_RMSPROP, false, false>(d, vec, k, s);
  } else {
    launch<HND_OPTIM_ADAGRAD, false, false>(d, vec, k, s);
  }
  return hnd::check_launch("hnd_optim_step_flat");
}

// Optimizer options on the device-resident segment table of rg_adam_multi_dev (include/recguru_hip.h): the squared global gradient
// norm with torch.nn.utils.clip_grad_norm_'s coefficient and the non-finite verdict in a control record (rg_grad_sqnorm_multi), and the
// Adam update that reads that record and applies coupled / decoupled weight decay (rg_adam_multi_dev2); the same update keeping an
// exponential moving average of the weights (rg_adam_multi_dev3) and the exchange of weights and averages (rg_ema_swap_multi).
//
// No float atomics and no accumulator shared between workgroups: every sum runs in an order fixed by the table alone, so this unit is
// compiled once and both libraries get the same bits from it.  The chain of roundings behind total_sq is written out beside
// RG_SQNORM_CHAIN in the header; a change to the loops below changes that macro.
#include <stdint.h>

#include "rg_common.hip.h"
#include "../../include/recguru_hip.h"

namespace {

constexpr int OPT_BLOCK = 256;

// partial[b] = sum of g[i]^2 over segment b.  The access pattern is adam_multi_dev_kernel's: 16-byte loads when p, g, m and v are all
// aligned (the same test, so that a segment takes the same route in both kernels), a scalar tail, the scalar walk otherwise.  A thread
// keeps four sums -- component j of its float4s, or element k & 3 of its scalar walk.
__global__ __launch_bounds__(OPT_BLOCK) void grad_sqnorm_seg_kernel(const rg_adam_seg_dev* __restrict__ segs, float* __restrict__ partial) {
  const rg_adam_seg_dev sg = segs[blockIdx.x];
  const float* __restrict__ g = sg.g;
  const long long n4 = (((uintptr_t)sg.p | (uintptr_t)g | (uintptr_t)sg.m | (uintptr_t)sg.v) & 15) ? 0 : (sg.n >> 2);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (long long i = threadIdx.x; i < n4; i += OPT_BLOCK) {
    const float4 g4 = reinterpret_cast<const float4*>(g)[i];
    a0 += g4.x * g4.x;
    a1 += g4.y * g4.y;
    a2 += g4.z * g4.z;
    a3 += g4.w * g4.w;
  }
  if (n4) {                                                        // tail of the vector route: at most three elements, one per thread
    const long long i = (n4 << 2) + threadIdx.x;
    if (i < sg.n) a0 += g[i] * g[i];
  } else {
    int k = 0;
    for (long long i = threadIdx.x; i < sg.n; i += OPT_BLOCK, ++k) {
      const float sq = g[i] * g[i];
      if ((k & 3) == 0) a0 += sq;
      else if ((k & 3) == 1) a1 += sq;
      else if ((k & 3) == 2) a2 += sq;
      else a3 += sq;
    }
  }
  float s = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);          // both partners add the same two values: every lane holds the wave's sum
  __shared__ float ws[OPT_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// One workgroup: total_sq = sum of partial[0 .. nsegs) in double -- thread t adds partial[t], partial[t + 256], ... in that order, then a
// tree over the threads -- and the control record.
__global__ __launch_bounds__(OPT_BLOCK) void grad_sqnorm_final_kernel(const float* __restrict__ partial, int nsegs, rg_adam_ctl* __restrict__ ctl,
                                                                    double max_norm, int skip_nonfinite) {
  __shared__ double sh[OPT_BLOCK];
  double s = 0.0;
  for (int i = threadIdx.x; i < nsegs; i += OPT_BLOCK) s += (double)partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = OPT_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double total = sh[0];
    const double nrm = sqrt(total);
    double coef = 1.0;
    if (max_norm > 0.0) {
      coef = max_norm / (nrm + 1e-6);
      if (coef > 1.0) coef = 1.0;                                  // (NaN stays NaN, as torch's clamp(max=1) leaves it)
    }
    const int skip = (skip_nonfinite && !isfinite(total)) ? 1 : 0;
    ctl->total_sq = total;
    ctl->norm = (float)nrm;
    ctl->coef = (float)coef;
    ctl->skip = skip;
    ctl->skipped = ctl->skipped + skip;                            // this launch is one workgroup and launches are ordered on the stream
  }
}

// adam_multi_dev_kernel (elementwise.hip) with the clip coefficient, the two decay forms and the skip: the body of a workgroup's segment,
// shared by adam_multi_dev2_kernel (EMA = false: e is never touched) and adam_multi_dev3_kernel (EMA = true) so that the two cannot
// drift.  The neutral call (ctl == NULL, wd == 0) takes none of the branches and evaluates adam_multi_dev_kernel's expressions on the
// same values.  EMA: behind the update e <- dt * e + omd * p_new on the value just stored to p; the 16-byte route then needs e aligned
// as well.  Both routes evaluate the same per-element expressions.
template <bool EMA>
__device__ __forceinline__ void adam_segment(const rg_adam_seg_dev& sg, float* __restrict__ e, double lr, double b1d, double b2d, float eps,
                                             float wd, float decay, const rg_adam_ctl* __restrict__ ctl, float dt, float omd) {
  const bool clip = ctl != nullptr;
  const float coef = clip ? ctl->coef : 1.f;
  const bool skip = clip && ctl->skip != 0;
  if (!skip) {
    const double st = (double)(sg.step + 1);
    const float step_lr = (float)(lr / (1.0 - pow(b1d, st)));
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow(b2d, st)));
    const float b1 = (float)b1d, b2 = (float)b2d;
    const bool coupled = wd != 0.f, decoupled = decay != 1.f;
    float* __restrict__ p = sg.p;
    const float* __restrict__ g = sg.g;
    float* __restrict__ m = sg.m;
    float* __restrict__ v = sg.v;
    const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (EMA ? (uintptr_t)e : (uintptr_t)0);
    const long long n4 = (bits & 15) ? 0 : (sg.n >> 2);
    for (long long i = threadIdx.x; i < n4; i += OPT_BLOCK) {
      const float4 g4 = reinterpret_cast<const float4*>(g)[i];
      float4 m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i], p4 = reinterpret_cast<float4*>(p)[i];
      float gg[4] = {g4.x, g4.y, g4.z, g4.w};
      float mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w}, pp[4] = {p4.x, p4.y, p4.z, p4.w};
      float ee[4] = {0.f, 0.f, 0.f, 0.f};
      if (EMA) {
        const float4 e4 = reinterpret_cast<float4*>(e)[i];
        ee[0] = e4.x, ee[1] = e4.y, ee[2] = e4.z, ee[3] = e4.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (clip) gg[j] = coef * gg[j];
        if (coupled) gg[j] = gg[j] + wd * pp[j];
        if (decoupled) pp[j] = pp[j] * decay;
        mm[j] = b1 * mm[j] + (1.f - b1) * gg[j];
        vv[j] = b2 * vv[j] + (1.f - b2) * gg[j] * gg[j];
        pp[j] = pp[j] - step_lr * (mm[j] / (sqrtf(vv[j]) * inv_bc2_sqrt + eps));
        if (EMA) ee[j] = dt * ee[j] + omd * pp[j];
      }
      reinterpret_cast<float4*>(m)[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
      reinterpret_cast<float4*>(v)[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
      reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
      if (EMA) reinterpret_cast<float4*>(e)[i] = make_float4(ee[0], ee[1], ee[2], ee[3]);
    }
    for (long long i = (n4 << 2) + threadIdx.x; i < sg.n; i += OPT_BLOCK) {
      float gi = g[i], pi = p[i];
      if (clip) gi = coef * gi;
      if (coupled) gi = gi + wd * pi;
      if (decoupled) pi = pi * decay;
      const float mi = b1 * m[i] + (1.f - b1) * gi;
      const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
      m[i] = mi;
      v[i] = vi;
      const float pn = pi - step_lr * (mi / (sqrtf(vi) * inv_bc2_sqrt + eps));
      p[i] = pn;
      if (EMA) e[i] = dt * e[i] + omd * pn;
    }
  }
}

__global__ __launch_bounds__(OPT_BLOCK) void adam_multi_dev2_kernel(rg_adam_seg_dev* __restrict__ segs, double lr, double b1d, double b2d,
                                                                  float eps, float wd, float decay, const rg_adam_ctl* __restrict__ ctl) {
  const rg_adam_seg_dev sg = segs[blockIdx.x];
  adam_segment<false>(sg, nullptr, lr, b1d, b2d, eps, wd, decay, ctl, 0.f, 0.f);
  __syncthreads();                                                 // every thread of the block has read its copy of sg
  if (threadIdx.x == 0) segs[blockIdx.x].step = sg.step + 1;       // a skipped step counts as a step
}

// adam_multi_dev2_kernel plus the exponential moving average ema[b] of segment b's weights, in the same pass: the new weight is in a
// register and the skip verdict is at hand.  The decay of this step comes from the segment's own count t = step + 1, in double, once per
// workgroup: d_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay.  A skipped step leaves the average alone as well.
__global__ __launch_bounds__(OPT_BLOCK) void adam_multi_dev3_kernel(rg_adam_seg_dev* __restrict__ segs, float* const* __restrict__ ema, double lr,
                                                                  double b1d, double b2d, float eps, float wd, float decay,
                                                                  const rg_adam_ctl* __restrict__ ctl, double ema_decay, int ema_warmup) {
  const rg_adam_seg_dev sg = segs[blockIdx.x];
  const double t = (double)(sg.step + 1);
  double d_t = ema_decay;
  if (ema_warmup) {
    const double w = (1.0 + t) / (10.0 + t);
    if (w < d_t) d_t = w;
  }
  adam_segment<true>(sg, ema[blockIdx.x], lr, b1d, b2d, eps, wd, decay, ctl, (float)d_t, (float)(1.0 - d_t));
  __syncthreads();                                                 // every thread of the block has read its copy of sg
  if (threadIdx.x == 0) segs[blockIdx.x].step = sg.step + 1;       // a skipped step counts as a step
}

// Exchange the two buffers of a pair as raw 32-bit words (no float ever exists: NaN payloads, -0.0 and denormals come through), one
// workgroup per pair; 16-byte moves when both buffers are aligned, a word tail behind them, the word walk otherwise.
__global__ __launch_bounds__(OPT_BLOCK) void ema_swap_kernel(const rg_ema_pair* __restrict__ pairs) {
  const rg_ema_pair pr = pairs[blockIdx.x];
  uint32_t* __restrict__ a = reinterpret_cast<uint32_t*>(pr.a);
  uint32_t* __restrict__ b = reinterpret_cast<uint32_t*>(pr.b);
  const long long n4 = (((uintptr_t)a | (uintptr_t)b) & 15) ? 0 : (pr.n >> 2);
  for (long long i = threadIdx.x; i < n4; i += OPT_BLOCK) {
    const uint4 x = reinterpret_cast<uint4*>(a)[i], y = reinterpret_cast<uint4*>(b)[i];
    reinterpret_cast<uint4*>(a)[i] = y;
    reinterpret_cast<uint4*>(b)[i] = x;
  }
  for (long long i = (n4 << 2) + threadIdx.x; i < pr.n; i += OPT_BLOCK) {
    const uint32_t x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

}  // namespace

extern "C" int rg_grad_sqnorm_multi(const rg_adam_seg_dev* segs_device, int nsegs, float* partial, rg_adam_ctl* ctl, double max_norm,
                                    int skip_nonfinite, void* stream) {
  if (nsegs < 1) return rg_set_error_msg(RG_ERR_INVALID, "grad_sqnorm_multi: nsegs < 1");
  if (!segs_device) return rg_set_error_msg(RG_ERR_INVALID, "grad_sqnorm_multi: null segment table");
  if (!partial || !ctl) return rg_set_error_msg(RG_ERR_INVALID, "grad_sqnorm_multi: null partial buffer or control record");
  if (!(max_norm >= 0.0)) return rg_set_error_msg(RG_ERR_INVALID, "grad_sqnorm_multi: max_norm < 0");
  hipLaunchKernelGGL(grad_sqnorm_seg_kernel, dim3(nsegs), dim3(OPT_BLOCK), 0, (hipStream_t)stream, segs_device, partial);
  RG_CHECK_LAUNCH();
  hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(OPT_BLOCK), 0, (hipStream_t)stream, (const float*)partial, nsegs, ctl, max_norm,
                     skip_nonfinite);
  RG_CHECK_LAUNCH();
  return 0;
}

extern "C" int rg_adam_multi_dev2(rg_adam_seg_dev* segs_device, int nsegs, double lr, double beta1, double beta2, double eps,
                                  double weight_decay, int decoupled, const rg_adam_ctl* ctl, void* stream) {
  if (nsegs < 1) return rg_set_error_msg(RG_ERR_INVALID, "adam_multi_dev2: nsegs < 1");
  if (!segs_device) return rg_set_error_msg(RG_ERR_INVALID, "adam_multi_dev2: null segment table");
  if (!(weight_decay >= 0.0)) return rg_set_error_msg(RG_ERR_INVALID, "adam_multi_dev2: weight_decay < 0");
  const float wd = decoupled ? 0.f : (float)weight_decay;
  const float decay = decoupled ? (float)(1.0 - lr * weight_decay) : 1.f;
  hipLaunchKernelGGL(adam_multi_dev2_kernel, dim3(nsegs), dim3(OPT_BLOCK), 0, (hipStream_t)stream, segs_device, lr, beta1, beta2, (float)eps,
                     wd, decay, ctl);
  RG_CHECK_LAUNCH();
  return 0;
}

extern "C" int rg_adam_multi_dev3(rg_adam_seg_dev* segs_device, float* const* ema_device, int nsegs, double lr, double beta1, double beta2,
                                  double eps, double weight_decay, int decoupled, const rg_adam_ctl* ctl, double ema_decay, int ema_warmup,
                                  void* stream) {
  if (nsegs < 1) return rg_set_error_msg(RG_ERR_INVALID, "adam_multi_dev3: nsegs < 1");
  if (!segs_device) return rg_set_error_msg(RG_ERR_INVALID, "adam_multi_dev3: null segment table");
  if (!ema_device) return rg_set_error_msg(RG_ERR_INVALID, "adam_multi_dev3: null average table");
  if (!(weight_decay >= 0.0)) return rg_set_error_msg(RG_ERR_INVALID, "adam_multi_dev3: weight_decay < 0");
  if (!(ema_decay >= 0.0 && ema_decay < 1.0)) return rg_set_error_msg(RG_ERR_INVALID, "adam_multi_dev3: ema_decay outside [0, 1)");
  const float wd = decoupled ? 0.f : (float)weight_decay;
  const float decay = decoupled ? (float)(1.0 - lr * weight_decay) : 1.f;
  hipLaunchKernelGGL(adam_multi_dev3_kernel, dim3(nsegs), dim3(OPT_BLOCK), 0, (hipStream_t)stream, segs_device, ema_device, lr, beta1, beta2,
                     (float)eps, wd, decay, ctl, ema_decay, ema_warmup);
  RG_CHECK_LAUNCH();
  return 0;
}

extern "C" int rg_ema_swap_multi(const rg_ema_pair* pairs_device, int npairs, void* stream) {
  if (npairs < 1) return rg_set_error_msg(RG_ERR_INVALID, "ema_swap_multi: npairs < 1");
  if (!pairs_device) return rg_set_error_msg(RG_ERR_INVALID, "ema_swap_multi: null pair table");
  hipLaunchKernelGGL(ema_swap_kernel, dim3(npairs), dim3(OPT_BLOCK), 0, (hipStream_t)stream, pairs_device);
  RG_CHECK_LAUNCH();
  return 0;
}

// Full-catalogue softmax cross-entropy over h @ W.T without the logits (AutoEnc4Rec.py:228-230 / AutoEnc4Rec_cross.py:216-220 with
// the loss of train_auto.py:44-51 / tools/utils.py:77-84, neg_sample=False; the evident intent of the reference, quirk Q15).
//
//   loss = sum_t m_t (lse_t - z_t[label_t]) / sum_t m_t,   z_t = W h_t over all C rows of W
//
// Three kernels, no float atomics (deterministic in both libraries; this unit does not include rg_det.hip.h):
//   full_ce_fwd_kernel<TRAIN>  token-major.  A workgroup owns FC_WAVES * TW live 16-row tiles (rg_live_tiles) and walks W once in
//       chunks of FC_CH rows staged in LDS for all its waves.  Per chunk: z^T = W_chunk . H^T on the matrix pipe (a wave's
//       accumulators hold 4 classes x 1 token per lane), an online max / sum-exp per token (exp2 with log2e folded in), and --
//       training form -- the P.V step of flash attention with W as V: dh^T += W_chunk^T . P^T, the probabilities fed back from
//       the accumulators as the B operand (stacked-accumulator mapping, rg_common.hip.h), the accumulator rescaled when the
//       running max moves.  The epilogue subtracts W[label], scales by m_t / sum(m) and writes dh (for an upstream gradient of 1),
//       lse, and one loss partial per workgroup.
//   full_ce_reduce_kernel      the partials in a fixed order -> sums[0].
//   full_ce_dw_kernel          vocab-major.  A workgroup owns FC_WAVES * CW 16-row tiles of W (held in registers) and walks every
//       live token in chunks of 32 staged in LDS: z = H_chunk . W_tile^T again, g = (exp(z - lse) - onehot) m gout / sum(m),
//       dW_tile^T += H_chunk^T . g (g fed back from the accumulators); each row of dW is read-modified-written once.
//
// Tiers: T = __bf16 (bf16 operands, f32 accumulation) and T = x3 (f32 buffers, split bf16 operands, three MFMAs per product: the
// bf16x3 tier and the f32 tier).  Rows of padded 16-row tiles are never computed (the forward zero-fills their dh rows; workgroups past
// the end of the live list return at once).
#include "rg_common.hip.h"
#include "../../include/recguru_hip.h"

namespace {

constexpr int FC_WAVES = 8;
constexpr int FC_THREADS = FC_WAVES * RG_WAVE;
constexpr int FC_CH = 32;                   // W rows per chunk of the forward, tokens per chunk of the dW kernel: one 32-deep k-step
constexpr int FC_LDT = FC_CH + 8;           // row pitch of a transposed LDS image (elements)
constexpr float FC_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float fc_max_g(float x) {      // over the four lanes 16 g + i that share i
  x = fmaxf(x, __shfl_xor(x, 16));
  return fmaxf(x, __shfl_xor(x, 32));
}
__device__ __forceinline__ float fc_sum_g(float x) {
  x += __shfl_xor(x, 16);
  return x + __shfl_xor(x, 32);
}

// first row of the e-th live 16-row tile, or -1
__device__ __forceinline__ long long fc_tile_row(const int* live16, int e) {
  return e < live16[0] ? (long long)live16[1 + e] * 16 : -1;
}

// one 8-element vector of rows [r0, r0 + ROWS) x D of src (rows >= nrows: zeros); v < ROWS * D / 8
template <typename T, int D>
__device__ __forceinline__ void fc_load_vec(Frag<T>& f, const T* src, long long row, long long nrows, int col) {
  if (row >= 0 && row < nrows) load_frag(f, src + row * D + col);
  else frag_zero(f);
}

// staged image of 32 rows x D: row-major [32][D + 8] and transposed [D][FC_LDT]
template <typename T, int D>
__device__ __forceinline__ void fc_stage(T* rm, T* tr, int r, int col, const Frag<T>& f) {
  *reinterpret_cast<Frag<T>*>(rm + r * (D + 8) + col) = f;
#pragma unroll
  for (int j = 0; j < 8; ++j) tr[(col + j) * FC_LDT + r] = f.v[j];
}

template <typename T, int D>
constexpr int fc_vecs_per_thread() { return (FC_CH * D / 8 + FC_THREADS - 1) / FC_THREADS; }

template <typename T, int D>
constexpr size_t fc_lds_bytes() { return 2 * (size_t)(FC_CH * (D + 8) + D * FC_LDT) * sizeof(T); }

// ------------------------------------------------------------------------------------------------
// forward (TRAIN: + dh for an upstream gradient of 1)
// ------------------------------------------------------------------------------------------------
template <typename T, int D, int TW, bool TRAIN>
__global__ __launch_bounds__(FC_THREADS) void full_ce_fwd_kernel(rg_full_ce_args a) {
  extern __shared__ __align__(16) unsigned char fc_lds[];
  T* const lds0 = reinterpret_cast<T*>(fc_lds);
  auto rm = [&](int b) { return lds0 + b * (FC_CH * (D + 8) + D * FC_LDT); };            // row-major image of buffer b
  auto tr = [&](int b) { return lds0 + b * (FC_CH * (D + 8) + D * FC_LDT) + FC_CH * (D + 8); };   // transposed image
  __shared__ float wsum[FC_WAVES];
  constexpr int KS = D / 32, DT = D / 16, NV = fc_vecs_per_thread<T, D>();
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.w);
  const long long C = a.C;
  const int e0 = blockIdx.x * FC_WAVES * TW;          // first list entry of this workgroup

  if constexpr (TRAIN) {
    // dh rows of the PADDED 16-row tiles among tiles [e0, e0 + FC_WAVES * TW) of the whole range (the grid covers every tile once):
    // zeros, by the criterion of rg_live_tiles (no mask != 0 in the tile); the live tiles' rows are written by the epilogue below
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) {
      const long long row = ((long long)e0 + wave * TW + tt) * 16 + i;
      const bool live = __ballot(row < a.n && a.mask[row] != 0.f) != 0;
      if (!live && row < a.n) {
        const float z[4] = {0.f, 0.f, 0.f, 0.f};
        T* dh = reinterpret_cast<T*>(a.dh) + row * D;
        for (int c = 4 * g; c < D; c += 16) store4(dh + c, z);
      }
    }
  }
  // the list holds fewer entries than tiles: a workgroup past its end has nothing to compute (its grid slot exists because the
  // host sizes the grid without reading the device-side count)
  if (e0 >= a.live16[0]) {
    if (tid == 0) a.partials[blockIdx.x] = 0.f;
    return;
  }

  long long row0[TW];
  Frag<T> hf[TW][KS];
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) {
    row0[tt] = fc_tile_row(a.live16, e0 + wave * TW + tt);
    const long long r = row0[tt] < 0 ? -1 : row0[tt] + i;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fc_load_vec<T, D>(hf[tt][ks], H, r, a.n, ks * 32 + 8 * g);
  }
  float mrun[TW], lrun[TW];
  f32x4 acc[TW][TRAIN ? DT : 1];
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) {
    mrun[tt] = -INFINITY;
    lrun[tt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < (TRAIN ? DT : 1); ++dt) acc[tt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  // the chunk's rows through registers: loaded one chunk ahead, staged behind the compute of the current one
  Frag<T> pre[NV];
  auto fetch = [&](long long c0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + v * FC_THREADS;
      if (idx < FC_CH * D / 8) fc_load_vec<T, D>(pre[v], W, c0 + idx / (D / 8), C, (idx % (D / 8)) * 8);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + v * FC_THREADS;
      if (idx < FC_CH * D / 8) fc_stage<T, D>(rm(buf), tr(buf), idx / (D / 8), (idx % (D / 8)) * 8, pre[v]);
    }
  };
  fetch(0);
  stage(0);
  __syncthreads();
  const int nch = (int)((C + FC_CH - 1) / FC_CH);
  for (int ch = 0; ch < nch; ++ch) {
    const int buf = ch & 1;
    const long long c0 = (long long)ch * FC_CH;
    if (ch + 1 < nch) fetch(c0 + FC_CH);
    // z^T for 32 classes x 16 tokens per token tile: lane (g, i), reg r = class c0 + 16 ct + 4 g + r, token i
    f32x4 s[TW][2];
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) s[tt][0] = s[tt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        Frag<T> wa;
        load_frag(wa, rm(buf) + (ct * 16 + i) * (D + 8) + ks * 32 + 8 * g);
#pragma unroll
        for (int tt = 0; tt < TW; ++tt) mma(wa, hf[tt][ks], s[tt][ct]);
      }
    }
    Frag<T> pb[TW];
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) {
      float cm = -INFINITY;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (c0 + ct * 16 + 4 * g + r >= C) s[tt][ct][r] = -INFINITY;
          cm = fmaxf(cm, s[tt][ct][r]);
        }
      const float mnew = fmaxf(mrun[tt], fc_max_g(cm));
      const float ml = mnew * FC_LOG2E;
      const float sc = __builtin_amdgcn_exp2f(mrun[tt] * FC_LOG2E - ml);
      mrun[tt] = mnew;
      float ls = 0.f;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[tt][ct][r], FC_LOG2E, -ml));
          s[tt][ct][r] = p;
          ls += p;
        }
      lrun[tt] = fmaf(lrun[tt], sc, ls);             // per-lane partial over its classes; summed over g in the epilogue
      if constexpr (TRAIN) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[tt][dt] *= sc;
        acc_to_frag(pb[tt], s[tt][0], s[tt][1]);
      }
    }
    if constexpr (TRAIN) {
      // dh^T (dcol x token) += W_chunk^T (dcol x class) . P^T (class x token)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        Frag<T> wt;
        const T* p = tr(buf) + (dt * 16 + i) * FC_LDT + 4 * g;
        load_frag_2x4(wt, p, p + 16);
#pragma unroll
        for (int tt = 0; tt < TW; ++tt) mma(wt, pb[tt], acc[tt][dt]);
      }
    }
    if (ch + 1 < nch) stage(buf ^ 1);
    __syncthreads();
  }

  // epilogue: lse, z[label] (f32 dot of the operands), loss partial, dh
  const float inv_cnt = TRAIN ? 1.f / a.sums[1] : 0.f;
  float part = 0.f;
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) {
    const float l = fc_sum_g(lrun[tt]);
    const long long row = row0[tt] < 0 ? -1 : row0[tt] + i;
    const bool ok = row >= 0 && row < a.n;
    long long lab = ok ? a.labels[row] : 0;
    lab = (lab >= 0 && lab < C) ? lab : 0;            // (an out-of-range label means row 0 here and in the dW kernel, never outside W)
    const float m = ok ? a.mask[row] : 0.f;
    const float lse = mrun[tt] + __logf(l);
    float zl = 0.f;
    float wl[DT][4];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      float hv[4];
      if (ok) {
        load4t(wl[dt], W + lab * D + dt * 16 + 4 * g);
        load4t(hv, H + row * D + dt * 16 + 4 * g);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) wl[dt][r] = hv[r] = 0.f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) zl = fmaf(hv[r], wl[dt][r], zl);
    }
    zl = fc_sum_g(zl);
    if (ok && g == 0) {
      a.lse[row] = lse;
      if (m != 0.f) part = fmaf(m, lse - zl, part);
    }
    if constexpr (TRAIN) {
      if (ok) {
        const float il = 1.f / l, sm = m * inv_cnt;
        T* dh = reinterpret_cast<T*>(a.dh) + row * D;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = m != 0.f ? (acc[tt][dt][r] * il - wl[dt][r]) * sm : 0.f;
          store4(dh + dt * 16 + 4 * g, v);
        }
      }
    }
  }
  part = wave_sum(part);
  if (lane == 0) wsum[wave] = part;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < FC_WAVES; ++w) t += wsum[w];
    a.partials[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void full_ce_reduce_kernel(const float* __restrict__ partials, int n, float* __restrict__ sums) {
  __shared__ float red[256];
  float t = 0.f;
  for (int k = threadIdx.x; k < n; k += 256) t += partials[k];
  red[threadIdx.x] = t;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[0] = red[0];
}

// ------------------------------------------------------------------------------------------------
// weight gradient, vocab-major: dW[c] += sum_t gout m_t / sum(m) (softmax_t[c] - [c == label_t]) h_t
// ------------------------------------------------------------------------------------------------
template <typename T, int D, int CW>
__global__ __launch_bounds__(FC_THREADS) void full_ce_dw_kernel(rg_full_ce_args a) {
  extern __shared__ __align__(16) unsigned char fc_lds[];
  T* const lds0 = reinterpret_cast<T*>(fc_lds);
  auto rm = [&](int b) { return lds0 + b * (FC_CH * (D + 8) + D * FC_LDT); };            // row-major image of buffer b
  auto tr = [&](int b) { return lds0 + b * (FC_CH * (D + 8) + D * FC_LDT) + FC_CH * (D + 8); };   // transposed image
  __shared__ float t_lse[2][FC_CH], t_coef[2][FC_CH];
  __shared__ long long t_lab[2][FC_CH];
  constexpr int KS = D / 32, DT = D / 16, NV = fc_vecs_per_thread<T, D>();
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.w);
  const long long C = a.C;
  const float gscale = (a.gout ? a.gout[0] : 1.f) / a.sums[1];

  long long cls0[CW];
  Frag<T> wf[CW][KS];
#pragma unroll
  for (int ct = 0; ct < CW; ++ct) {
    cls0[ct] = ((long long)blockIdx.x * FC_WAVES * CW + wave * CW + ct) * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fc_load_vec<T, D>(wf[ct][ks], W, cls0[ct] + i, C, ks * 32 + 8 * g);
  }
  f32x4 acc[CW][DT];
#pragma unroll
  for (int ct = 0; ct < CW; ++ct)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[ct][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // a chunk = list entries 2 k, 2 k + 1 (32 token rows)
  Frag<T> pre[NV];
  float p_lse = 0.f, p_coef = 0.f;
  long long p_lab = -1;
  auto fetch = [&](int k) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + v * FC_THREADS;
      if (idx < FC_CH * D / 8) {
        const int r = idx / (D / 8);
        const long long t0 = fc_tile_row(a.live16, 2 * k + (r >> 4));
        fc_load_vec<T, D>(pre[v], H, t0 < 0 ? -1 : t0 + (r & 15), a.n, (idx % (D / 8)) * 8);
      }
    }
    if (tid < FC_CH) {
      const long long t0 = fc_tile_row(a.live16, 2 * k + (tid >> 4));
      const long long row = t0 < 0 ? -1 : t0 + (tid & 15);
      const bool ok = row >= 0 && row < a.n;
      const float m = ok ? a.mask[row] : 0.f;
      p_coef = m * gscale;
      p_lse = (ok && m != 0.f) ? a.lse[row] : 0.f;
      const long long lab = (ok && m != 0.f) ? a.labels[row] : -1;
      p_lab = lab < 0 ? -1 : (lab < C ? lab : 0);          // out-of-range labels: row 0, as in the forward
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + v * FC_THREADS;
      if (idx < FC_CH * D / 8) fc_stage<T, D>(rm(buf), tr(buf), idx / (D / 8), (idx % (D / 8)) * 8, pre[v]);
    }
    if (tid < FC_CH) {
      t_lse[buf][tid] = p_lse;
      t_coef[buf][tid] = p_coef;
      t_lab[buf][tid] = p_lab;
    }
  };
  const int nch = (a.live16[0] + 1) >> 1;
  if (nch > 0) {
    fetch(0);
    stage(0);
  }
  __syncthreads();
  for (int k = 0; k < nch; ++k) {
    const int buf = k & 1;
    if (k + 1 < nch) fetch(k + 1);
    // z for 32 tokens x 16 classes per class tile: lane (g, i), reg r = token 16 tt + 4 g + r, class cls0 + i
    f32x4 s[2][CW];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int ct = 0; ct < CW; ++ct) s[tt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        Frag<T> ha;
        load_frag(ha, rm(buf) + (tt * 16 + i) * (D + 8) + ks * 32 + 8 * g);
#pragma unroll
        for (int ct = 0; ct < CW; ++ct) mma(ha, wf[ct][ks], s[tt][ct]);
      }
    Frag<T> gb[CW];
#pragma unroll
    for (int ct = 0; ct < CW; ++ct) {
      const long long c = cls0[ct] + i;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = tt * 16 + 4 * g + r;
          const float co = t_coef[buf][t];
          const float p = __builtin_amdgcn_exp2f((s[tt][ct][r] - t_lse[buf][t]) * FC_LOG2E) - (t_lab[buf][t] == c ? 1.f : 0.f);
          s[tt][ct][r] = co != 0.f ? p * co : 0.f;
        }
      acc_to_frag(gb[ct], s[0][ct], s[1][ct]);
    }
    // dW^T (dcol x class) += H_chunk^T (dcol x token) . g (token x class)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      Frag<T> ht;
      const T* p = tr(buf) + (dt * 16 + i) * FC_LDT + 4 * g;
      load_frag_2x4(ht, p, p + 16);
#pragma unroll
      for (int ct = 0; ct < CW; ++ct) mma(ht, gb[ct], acc[ct][dt]);
    }
    if (k + 1 < nch) stage(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int ct = 0; ct < CW; ++ct) {
    const long long c = cls0[ct] + i;
    if (c >= C) continue;
    float* dst = a.dw + c * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      float v[4];
      load4f(v, dst + dt * 16 + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += acc[ct][dt][r];
      store4(dst + dt * 16 + 4 * g, v);
    }
  }
}

template <typename T, int D> constexpr int fc_tw() { return D <= 128 ? 2 : 1; }
template <typename T, int D> constexpr int fc_cw() { return D <= 128 ? 2 : 1; }

template <typename T, int D, bool TRAIN>
int launch_fwd(const rg_full_ce_args& a, hipStream_t s) {
  constexpr int TW = fc_tw<T, D>();
  const long long tiles = (a.n + 15) / 16;
  const int nwg = (int)((tiles + FC_WAVES * TW - 1) / (FC_WAVES * TW));
  const size_t lds = fc_lds_bytes<T, D>();
  auto k = full_ce_fwd_kernel<T, D, TW, TRAIN>;
  hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, dim3(nwg), dim3(FC_THREADS), lds, s, a);
  hipLaunchKernelGGL(full_ce_reduce_kernel, dim3(1), dim3(256), 0, s, a.partials, nwg, a.sums);
  RG_CHECK_LAUNCH();
  return 0;
}

template <typename T, int D>
int launch_dw(const rg_full_ce_args& a, hipStream_t s) {
  constexpr int CW = fc_cw<T, D>();
  const int nwg = (int)((a.C + FC_WAVES * CW * 16 - 1) / (FC_WAVES * CW * 16));
  const size_t lds = fc_lds_bytes<T, D>();
  auto k = full_ce_dw_kernel<T, D, CW>;
  hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, dim3(nwg), dim3(FC_THREADS), lds, s, a);
  RG_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int dispatch_fwd(const rg_full_ce_args& a, int train, hipStream_t s) {
  switch (a.d) {
    case 64: return train ? launch_fwd<T, 64, true>(a, s) : launch_fwd<T, 64, false>(a, s);
    case 128: return train ? launch_fwd<T, 128, true>(a, s) : launch_fwd<T, 128, false>(a, s);
    case 256: return train ? launch_fwd<T, 256, true>(a, s) : launch_fwd<T, 256, false>(a, s);
  }
  return rg_set_error_msg(RG_ERR_UNSUPPORTED, "full_ce: d must be 64, 128 or 256");
}

template <typename T>
int dispatch_dw(const rg_full_ce_args& a, hipStream_t s) {
  switch (a.d) {
    case 64: return launch_dw<T, 64>(a, s);
    case 128: return launch_dw<T, 128>(a, s);
    case 256: return launch_dw<T, 256>(a, s);
  }
  return rg_set_error_msg(RG_ERR_UNSUPPORTED, "full_ce: d must be 64, 128 or 256");
}

int check_args(const rg_full_ce_args* a, const char* what) {
  static thread_local char msg[160];
  if (!a || !a->h || !a->w || !a->labels || !a->mask || !a->live16 || !a->lse || !a->sums) {
    snprintf(msg, sizeof(msg), "%s: h, w, labels, mask, live16, lse and sums are required", what);
    return rg_set_error_msg(RG_ERR_INVALID, msg);
  }
  if (a->C <= 0 || a->C >= (1LL << 31)) {
    snprintf(msg, sizeof(msg), "%s: C must be in [1, 2^31)", what);
    return rg_set_error_msg(RG_ERR_INVALID, msg);
  }
  return 0;
}

}  // namespace

extern "C" int rg_full_ce_supported(int d, int dtype) {
  return (d == 64 || d == 128 || d == 256) && (dtype == RG_BF16 || dtype == RG_X3);
}

extern "C" int rg_full_ce_fwd(const rg_full_ce_args* a, int train, int dtype, void* stream) {
  if (a && a->n <= 0) return 0;
  if (int e = check_args(a, "full_ce_fwd")) return e;
  if (!a->partials || (train && !a->dh)) return rg_set_error_msg(RG_ERR_INVALID, "full_ce_fwd: partials (and dh for the training form) are required");
  if (dtype == RG_BF16) return dispatch_fwd<__bf16>(*a, train, (hipStream_t)stream);
  if (dtype == RG_X3) return dispatch_fwd<x3>(*a, train, (hipStream_t)stream);
  return rg_set_error_msg(RG_ERR_UNSUPPORTED, "full_ce_fwd: dtype must be RG_BF16 or RG_X3");
}

extern "C" int rg_full_ce_dw(const rg_full_ce_args* a, int dtype, void* stream) {
  if (a && a->n <= 0) return 0;
  if (int e = check_args(a, "full_ce_dw")) return e;
  if (!a->dw) return rg_set_error_msg(RG_ERR_INVALID, "full_ce_dw: dw is required");
  if (dtype == RG_BF16) return dispatch_dw<__bf16>(*a, (hipStream_t)stream);
  if (dtype == RG_X3) return dispatch_dw<x3>(*a, (hipStream_t)stream);
  return rg_set_error_msg(RG_ERR_UNSUPPORTED, "full_ce_dw: dtype must be RG_BF16 or RG_X3");
}

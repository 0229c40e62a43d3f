// Sampled softmax over ONE candidate set shared by every position of the call: the structure of full_ce.hip over the
// C gathered rows E[S_c] of the item table instead of a whole weight matrix.
//
//   z_pos  = h_t . E[y_t] (+ pos_bias[t]),   z_c = h_t . E[S_c] (+ cand_bias[c]) for every c with S_c != y_t
//   loss   = sum_t m_t (log(exp(z_pos) + sum_c exp(z_c)) - z_pos) / sum_t m_t
//
// Kernels, no float atomics (deterministic in both libraries; this unit does not include rg_det.hip.h):
//   shared_ce_gather_kernel     wc [C, d] = E[S_c]: the compact operand both products read.
//   shared_ce_fwd_kernel<TRAIN> token-major, full_ce_fwd_kernel's walk over wc in LDS-staged chunks of SC_CH rows.  The online max /
//       sum-exp of a position starts at (z_pos, 1) -- z_pos an f32 gather-dot of the operands -- and a candidate equal to the
//       position's own target enters as -inf ("accidental hit").  Training form: dh^T += wc_chunk^T . P^T with the probabilities fed
//       back from the accumulators; the epilogue adds (p_pos - 1) E[y_t], scales by m_t / sum(m) and writes dh, lse, the target
//       coefficient (p_pos - 1) m_t / sum(m) and one loss partial per workgroup.
//   shared_ce_reduce_kernel     the partials in a fixed order -> sums[0].
//   shared_ce_dw_kernel         candidate-major, full_ce_dw_kernel's tile (SC_WAVES * CW 16-row tiles of wc in registers) -- but the walk
//       over the live rows is SPLIT across gridDim.y workgroups (C = 1024 would otherwise be 4 workgroups on 256 CUs); split s owns a
//       contiguous range of 32-row chunks of the live list and stores its [C, d] f32 partial, no read-modify-write.
//   shared_ce_scatter_kernel    dE[S_c] += the splits' partials summed in split order: ids are unique, one lane per dE element.
//   shared_ce_scale_rows_kernel hs = coef_pos * gout * h and the clamped targets: the operands of the embedding scatter that carries
//       the target route (rg_embed_scatter_bwd[_binned], run by the caller on hs).
// The number of splits depends on (n, C, d) alone and a split's range on the live list alone: results repeat bit for bit.
//
// Tiers: T = __bf16 and T = x3 as in full_ce.hip.  Rows of padded 16-row tiles are never computed.
#include <vector>
#include "rg_common.hip.h"
#include "../../include/recguru_hip.h"

namespace {

constexpr int SC_WAVES = 8;
constexpr int SC_THREADS = SC_WAVES * RG_WAVE;
constexpr int SC_CH = 32;                   // wc rows per chunk of the forward, tokens per chunk of the dw kernel: one 32-deep k-step
constexpr int SC_LDT = SC_CH + 8;           // row pitch of a transposed LDS image (elements)
constexpr float SC_LOG2E = 1.4426950408889634f;
constexpr int SC_TARGET_WGS = 512;          // dw grid the splits aim at: two workgroups per CU

__device__ __forceinline__ float sc_max_g(float x) {      // over the four lanes 16 g + i that share i
  x = fmaxf(x, __shfl_xor(x, 16));
  return fmaxf(x, __shfl_xor(x, 32));
}
__device__ __forceinline__ float sc_sum_g(float x) {
  x += __shfl_xor(x, 16);
  return x + __shfl_xor(x, 32);
}

// first row of the e-th live 16-row tile, or -1
__device__ __forceinline__ long long sc_tile_row(const int* live16, int e) {
  return e < live16[0] ? (long long)live16[1 + e] * 16 : -1;
}

template <typename T, int D>
__device__ __forceinline__ void sc_load_vec(Frag<T>& f, const T* src, long long row, long long nrows, int col) {
  if (row >= 0 && row < nrows) load_frag(f, src + row * D + col);
  else frag_zero(f);
}

// staged image of 32 rows x D: row-major [32][D + 8] and transposed [D][SC_LDT]
template <typename T, int D>
__device__ __forceinline__ void sc_stage(T* rm, T* tr, int r, int col, const Frag<T>& f) {
  *reinterpret_cast<Frag<T>*>(rm + r * (D + 8) + col) = f;
#pragma unroll
  for (int j = 0; j < 8; ++j) tr[(col + j) * SC_LDT + r] = f.v[j];
}

template <typename T, int D>
constexpr int sc_vecs_per_thread() { return (SC_CH * D / 8 + SC_THREADS - 1) / SC_THREADS; }

template <typename T, int D>
constexpr size_t sc_lds_bytes() { return 2 * (size_t)(SC_CH * (D + 8) + D * SC_LDT) * sizeof(T); }

// a label as the row of the table it stands for: outside [0, rows) means row 0 (as in full_ce.hip, never outside the table)
__device__ __forceinline__ long long sc_label(long long lab, long long rows) { return (lab >= 0 && lab < rows) ? lab : 0; }

// ------------------------------------------------------------------------------------------------
// wc[c] = E[S_c]
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void shared_ce_gather_kernel(const T* __restrict__ table, const int64_t* __restrict__ cand,
                                                               T* __restrict__ wc, long long C, long long rows, int d) {
  const int vpr = d / 8;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= C * vpr) return;
  const long long c = idx / vpr;
  const int col = (int)(idx % vpr) * 8;
  const long long r = cand[c];
  Frag<T> f;
  if (r >= 0 && r < rows) load_frag(f, table + r * d + col);       // (the host has checked the ids; this guards the table all the same)
  else frag_zero(f);
  *reinterpret_cast<Frag<T>*>(wc + c * d + col) = f;
}

// ------------------------------------------------------------------------------------------------
// forward (TRAIN: + dh and the target coefficient for an upstream gradient of 1)
// ------------------------------------------------------------------------------------------------
template <typename T, int D, int TW, bool TRAIN>
__global__ __launch_bounds__(SC_THREADS) void shared_ce_fwd_kernel(rg_shared_ce_args a) {
  extern __shared__ __align__(16) unsigned char sc_lds[];
  T* const lds0 = reinterpret_cast<T*>(sc_lds);
  auto rm = [&](int b) { return lds0 + b * (SC_CH * (D + 8) + D * SC_LDT); };            // row-major image of buffer b
  auto tr = [&](int b) { return lds0 + b * (SC_CH * (D + 8) + D * SC_LDT) + SC_CH * (D + 8); };   // transposed image
  __shared__ float wsum[SC_WAVES];
  __shared__ long long c_id[2][SC_CH];      // the chunk's candidate ids (-1 past C) and biases
  __shared__ float c_bias[2][SC_CH];
  constexpr int KS = D / 32, DT = D / 16, NV = sc_vecs_per_thread<T, D>();
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ E = reinterpret_cast<const T*>(a.table);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.wc);
  const long long C = a.C;
  const int e0 = blockIdx.x * SC_WAVES * TW;          // first list entry of this workgroup

  if constexpr (TRAIN) {
    // dh rows and target coefficients of the PADDED 16-row tiles among tiles [e0, e0 + SC_WAVES * TW) of the whole range (the grid
    // covers every tile once): zeros, by the criterion of rg_live_tiles; the live tiles' rows are written by the epilogue below
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) {
      const long long row = ((long long)e0 + wave * TW + tt) * 16 + i;
      const bool live = __ballot(row < a.n && a.mask[row] != 0.f) != 0;
      if (!live && row < a.n) {
        const float z[4] = {0.f, 0.f, 0.f, 0.f};
        T* dh = reinterpret_cast<T*>(a.dh) + row * D;
        for (int c = 4 * g; c < D; c += 16) store4(dh + c, z);
        if (g == 0) a.coef_pos[row] = 0.f;
      }
    }
  }
  if (e0 >= a.live16[0]) {
    if (tid == 0) a.partials[blockIdx.x] = 0.f;
    return;
  }

  long long row0[TW], lab[TW];
  Frag<T> hf[TW][KS];
  float zpos[TW];
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) {
    row0[tt] = sc_tile_row(a.live16, e0 + wave * TW + tt);
    const long long r = row0[tt] < 0 ? -1 : row0[tt] + i;
    const bool ok = r >= 0 && r < a.n;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) sc_load_vec<T, D>(hf[tt][ks], H, r, a.n, ks * 32 + 8 * g);
    // z_pos: f32 dot of the operands, every lane of a token column ends up with the whole sum
    lab[tt] = sc_label(ok ? a.labels[r] : 0, a.rows);
    float zl = 0.f;
    if (ok) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        float wl[4], hv[4];
        load4t(wl, E + lab[tt] * D + dt * 16 + 4 * g);
        load4t(hv, H + r * D + dt * 16 + 4 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) zl = fmaf(hv[q], wl[q], zl);
      }
    }
    zl = sc_sum_g(zl);
    zpos[tt] = zl + ((ok && a.pos_bias) ? a.pos_bias[r] : 0.f);
  }
  // the sum starts with the target's own term: running max z_pos, exp(z_pos - max) = 1 (held by the g == 0 lane of the column)
  float mrun[TW], lrun[TW];
  f32x4 acc[TW][TRAIN ? DT : 1];
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) {
    mrun[tt] = zpos[tt];
    lrun[tt] = g == 0 ? 1.f : 0.f;
#pragma unroll
    for (int dt = 0; dt < (TRAIN ? DT : 1); ++dt) acc[tt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  // the chunk's rows through registers: loaded one chunk ahead, staged behind the compute of the current one
  Frag<T> pre[NV];
  long long p_id = -1;
  float p_bias = 0.f;
  auto fetch = [&](long long c0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + v * SC_THREADS;
      if (idx < SC_CH * D / 8) sc_load_vec<T, D>(pre[v], W, c0 + idx / (D / 8), C, (idx % (D / 8)) * 8);
    }
    if (tid < SC_CH) {
      const long long c = c0 + tid;
      p_id = c < C ? a.cand[c] : -1;
      p_bias = (c < C && a.cand_bias) ? a.cand_bias[c] : 0.f;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + v * SC_THREADS;
      if (idx < SC_CH * D / 8) sc_stage<T, D>(rm(buf), tr(buf), idx / (D / 8), (idx % (D / 8)) * 8, pre[v]);
    }
    if (tid < SC_CH) {
      c_id[buf][tid] = p_id;
      c_bias[buf][tid] = p_bias;
    }
  };
  fetch(0);
  stage(0);
  __syncthreads();
  const int nch = (int)((C + SC_CH - 1) / SC_CH);
  for (int ch = 0; ch < nch; ++ch) {
    const int buf = ch & 1;
    const long long c0 = (long long)ch * SC_CH;
    if (ch + 1 < nch) fetch(c0 + SC_CH);
    // z^T for 32 candidates x 16 tokens per token tile: lane (g, i), reg r = candidate c0 + 16 ct + 4 g + r, token i
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
    long long cid[2][4];
    float cb[2][4];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        cid[ct][r] = c_id[buf][ct * 16 + 4 * g + r];
        cb[ct][r] = c_bias[buf][ct * 16 + 4 * g + r];
      }
    Frag<T> pb[TW];
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) {
      float cm = -INFINITY;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // past the end of S, or the position's own target: out of the sum
          s[tt][ct][r] = (cid[ct][r] < 0 || cid[ct][r] == lab[tt]) ? -INFINITY : s[tt][ct][r] + cb[ct][r];
          cm = fmaxf(cm, s[tt][ct][r]);
        }
      const float mnew = fmaxf(mrun[tt], sc_max_g(cm));
      const float ml = mnew * SC_LOG2E;
      // (an unmoved max rescales by exactly 1: under fp contraction the difference below is the rounding residue of ml, not 0)
      const float sc = mnew == mrun[tt] ? 1.f : __builtin_amdgcn_exp2f(mrun[tt] * SC_LOG2E - ml);
      mrun[tt] = mnew;
      float ls = 0.f;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[tt][ct][r], SC_LOG2E, -ml));
          s[tt][ct][r] = p;
          ls += p;
        }
      lrun[tt] = fmaf(lrun[tt], sc, ls);             // per-lane partial over its candidates; summed over g in the epilogue
      if constexpr (TRAIN) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[tt][dt] *= sc;
        acc_to_frag(pb[tt], s[tt][0], s[tt][1]);
      }
    }
    if constexpr (TRAIN) {
      // dh^T (dcol x token) += wc_chunk^T (dcol x candidate) . P^T (candidate x token)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        Frag<T> wt;
        const T* p = tr(buf) + (dt * 16 + i) * SC_LDT + 4 * g;
        load_frag_2x4(wt, p, p + 16);
#pragma unroll
        for (int tt = 0; tt < TW; ++tt) mma(wt, pb[tt], acc[tt][dt]);
      }
    }
    if (ch + 1 < nch) stage(buf ^ 1);
    __syncthreads();
  }

  // epilogue: lse, loss partial, dh, target coefficient
  const float inv_cnt = TRAIN ? 1.f / a.sums[1] : 0.f;
  float part = 0.f;
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) {
    const float l = sc_sum_g(lrun[tt]);
    const long long row = row0[tt] < 0 ? -1 : row0[tt] + i;
    const bool ok = row >= 0 && row < a.n;
    const float m = ok ? a.mask[row] : 0.f;
    const float lse = mrun[tt] + __logf(l);
    if (ok && g == 0) {
      a.lse[row] = lse;
      if (m != 0.f) part = fmaf(m, lse - zpos[tt], part);
    }
    if constexpr (TRAIN) {
      if (ok) {
        const float il = 1.f / l, sm = m * inv_cnt;
        const float ppos1 = __builtin_amdgcn_exp2f((zpos[tt] - mrun[tt]) * SC_LOG2E) * il - 1.f;      // p_pos - 1
        if (g == 0) a.coef_pos[row] = m != 0.f ? ppos1 * sm : 0.f;
        T* dh = reinterpret_cast<T*>(a.dh) + row * D;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          float wl[4], v[4];
          load4t(wl, E + lab[tt] * D + dt * 16 + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = m != 0.f ? fmaf(ppos1, wl[r], acc[tt][dt][r] * il) * sm : 0.f;
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
    for (int w = 0; w < SC_WAVES; ++w) t += wsum[w];
    a.partials[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void shared_ce_reduce_kernel(const float* __restrict__ partials, int n, float* __restrict__ sums) {
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
// candidate part of the table gradient: part[split][c] = sum_{t in split} gout m_t / sum(m) p_{t,c} h_t
// ------------------------------------------------------------------------------------------------
template <typename T, int D, int CW>
__global__ __launch_bounds__(SC_THREADS) void shared_ce_dw_kernel(rg_shared_ce_args a) {
  extern __shared__ __align__(16) unsigned char sc_lds[];
  T* const lds0 = reinterpret_cast<T*>(sc_lds);
  auto rm = [&](int b) { return lds0 + b * (SC_CH * (D + 8) + D * SC_LDT); };            // row-major image of buffer b
  auto tr = [&](int b) { return lds0 + b * (SC_CH * (D + 8) + D * SC_LDT) + SC_CH * (D + 8); };   // transposed image
  __shared__ float t_lse[2][SC_CH], t_coef[2][SC_CH];
  __shared__ long long t_lab[2][SC_CH];
  constexpr int KS = D / 32, DT = D / 16, NV = sc_vecs_per_thread<T, D>();
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.wc);
  const long long C = a.C;
  const float gscale = (a.gout ? a.gout[0] : 1.f) / a.sums[1];

  long long cls0[CW], cid[CW];
  float cb[CW];
  Frag<T> wf[CW][KS];
#pragma unroll
  for (int ct = 0; ct < CW; ++ct) {
    cls0[ct] = ((long long)blockIdx.x * SC_WAVES * CW + wave * CW + ct) * 16;
    const long long c = cls0[ct] + i;
    cid[ct] = c < C ? a.cand[c] : -1;
    cb[ct] = (c < C && a.cand_bias) ? a.cand_bias[c] : 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) sc_load_vec<T, D>(wf[ct][ks], W, c, C, ks * 32 + 8 * g);
  }
  f32x4 acc[CW][DT];
#pragma unroll
  for (int ct = 0; ct < CW; ++ct)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[ct][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // a chunk = list entries 2 k, 2 k + 1 (32 token rows); this split's chunks are [k0, k1)
  Frag<T> pre[NV];
  float p_lse = 0.f, p_coef = 0.f;
  long long p_lab = -1;
  auto fetch = [&](int k) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + v * SC_THREADS;
      if (idx < SC_CH * D / 8) {
        const int r = idx / (D / 8);
        const long long t0 = sc_tile_row(a.live16, 2 * k + (r >> 4));
        sc_load_vec<T, D>(pre[v], H, t0 < 0 ? -1 : t0 + (r & 15), a.n, (idx % (D / 8)) * 8);
      }
    }
    if (tid < SC_CH) {
      const long long t0 = sc_tile_row(a.live16, 2 * k + (tid >> 4));
      const long long row = t0 < 0 ? -1 : t0 + (tid & 15);
      const bool ok = row >= 0 && row < a.n;
      const float m = ok ? a.mask[row] : 0.f;
      p_coef = m * gscale;
      p_lse = (ok && m != 0.f) ? a.lse[row] : 0.f;
      p_lab = (ok && m != 0.f) ? sc_label(a.labels[row], a.rows) : -2;       // (-2: no candidate slot, a real one or the -1 of a tail, equals it)
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + v * SC_THREADS;
      if (idx < SC_CH * D / 8) sc_stage<T, D>(rm(buf), tr(buf), idx / (D / 8), (idx % (D / 8)) * 8, pre[v]);
    }
    if (tid < SC_CH) {
      t_lse[buf][tid] = p_lse;
      t_coef[buf][tid] = p_coef;
      t_lab[buf][tid] = p_lab;
    }
  };
  const int nch = (a.live16[0] + 1) >> 1;
  const int per = (nch + (int)gridDim.y - 1) / (int)gridDim.y;
  const int k0 = min(nch, (int)blockIdx.y * per), k1 = min(nch, k0 + per);
  if (k0 < k1) {
    fetch(k0);
    stage(0);
  }
  __syncthreads();
  for (int k = k0; k < k1; ++k) {
    const int buf = (k - k0) & 1;
    if (k + 1 < k1) fetch(k + 1);
    // z for 32 tokens x 16 candidates per candidate tile: lane (g, i), reg r = token 16 tt + 4 g + r, candidate cls0 + i
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
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = tt * 16 + 4 * g + r;
          const float co = t_coef[buf][t];
          const float p = __builtin_amdgcn_exp2f((s[tt][ct][r] + cb[ct] - t_lse[buf][t]) * SC_LOG2E);
          s[tt][ct][r] = (co != 0.f && t_lab[buf][t] != cid[ct]) ? p * co : 0.f;      // an accidental hit is not in the position's sum
        }
      acc_to_frag(gb[ct], s[0][ct], s[1][ct]);
    }
    // part^T (dcol x candidate) += H_chunk^T (dcol x token) . g (token x candidate)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      Frag<T> ht;
      const T* p = tr(buf) + (dt * 16 + i) * SC_LDT + 4 * g;
      load_frag_2x4(ht, p, p + 16);
#pragma unroll
      for (int ct = 0; ct < CW; ++ct) mma(ht, gb[ct], acc[ct][dt]);
    }
    if (k + 1 < k1) stage(buf ^ 1);
    __syncthreads();
  }
  // every split stores its whole tile (zeros when its range is empty): the scatter sums all gridDim.y of them
#pragma unroll
  for (int ct = 0; ct < CW; ++ct) {
    const long long c = cls0[ct] + i;
    if (c >= C) continue;
    float* dst = a.dw_part + ((long long)blockIdx.y * C + c) * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const float v[4] = {acc[ct][dt][0], acc[ct][dt][1], acc[ct][dt][2], acc[ct][dt][3]};
      store4(dst + dt * 16 + 4 * g, v);
    }
  }
}

// dE[S_c] += sum over the splits, in split order; ids are unique: one lane per four elements of dE, no atomics
__global__ __launch_bounds__(256) void shared_ce_scatter_kernel(const float* __restrict__ part, const int64_t* __restrict__ cand,
                                                                float* __restrict__ dE, long long C, long long rows, int d, int splits) {
  const int vpr = d / 4;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= C * vpr) return;
  const long long c = idx / vpr;
  const int col = (int)(idx % vpr) * 4;
  const long long r = cand[c];
  if (r < 0 || r >= rows) return;
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < splits; ++s) {
    float v[4];
    load4f(v, part + ((long long)s * C + c) * d + col);
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] += v[q];
  }
  float o[4];
  load4f(o, dE + r * d + col);
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] += t[q];
  store4(dE + r * d + col, o);
}

// hs[t] = coef_pos[t] * gout * h[t] (zeros on masked rows) and tgt[t] = the table row label t stands for
template <typename T>
__global__ __launch_bounds__(256) void shared_ce_scale_rows_kernel(const T* __restrict__ h, const float* __restrict__ coef_pos,
                                                                   const float* __restrict__ mask, const int64_t* __restrict__ labels,
                                                                   const float* __restrict__ gout, T* __restrict__ hs,
                                                                   int64_t* __restrict__ tgt, long long n, long long rows, int d) {
  const int vpr = d / 4;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * vpr) return;
  const long long t = idx / vpr;
  const int col = (int)(idx % vpr) * 4;
  const float m = mask[t];
  const float co = m != 0.f ? coef_pos[t] * (gout ? gout[0] : 1.f) : 0.f;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (m != 0.f) {
    load4t(v, h + t * d + col);
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] *= co;
  }
  store4(hs + t * d + col, v);
  if (col == 0) tgt[t] = sc_label(labels[t], rows);
}

template <typename T, int D> constexpr int sc_tw() { return D <= 128 ? 2 : 1; }
template <typename T, int D> constexpr int sc_cw() { return D <= 128 ? 2 : 1; }

// the number of splits of the dw walk: from (n, C, d) alone
int sc_splits(long long n, long long C, int d) {
  const int cw = d <= 128 ? 2 : 1;
  const long long ncblk = (C + SC_WAVES * cw * 16 - 1) / (SC_WAVES * cw * 16);
  const long long tiles = (n + 15) / 16;
  long long s = SC_TARGET_WGS / ncblk;
  const long long cap = (tiles + 7) / 8;          // at least four 32-row chunks per split when every tile is live
  if (s > cap) s = cap;
  return (int)(s < 1 ? 1 : s);
}

template <typename T, int D, bool TRAIN>
int launch_fwd(const rg_shared_ce_args& a, hipStream_t s) {
  constexpr int TW = sc_tw<T, D>();
  const long long tiles = (a.n + 15) / 16;
  const int nwg = (int)((tiles + SC_WAVES * TW - 1) / (SC_WAVES * TW));
  const size_t lds = sc_lds_bytes<T, D>();
  const long long nv = a.C * (D / 8);
  hipLaunchKernelGGL(shared_ce_gather_kernel<T>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const T*>(a.table),
                     a.cand, reinterpret_cast<T*>(a.wc), a.C, a.rows, D);
  auto k = shared_ce_fwd_kernel<T, D, TW, TRAIN>;
  hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, dim3(nwg), dim3(SC_THREADS), lds, s, a);
  hipLaunchKernelGGL(shared_ce_reduce_kernel, dim3(1), dim3(256), 0, s, a.partials, nwg, a.sums);
  RG_CHECK_LAUNCH();
  return 0;
}

template <typename T, int D>
int launch_bwd(const rg_shared_ce_args& a, hipStream_t s) {
  constexpr int CW = sc_cw<T, D>();
  const int ncblk = (int)((a.C + SC_WAVES * CW * 16 - 1) / (SC_WAVES * CW * 16));
  const int splits = sc_splits(a.n, a.C, D);
  const size_t lds = sc_lds_bytes<T, D>();
  auto k = shared_ce_dw_kernel<T, D, CW>;
  hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, dim3(ncblk, splits), dim3(SC_THREADS), lds, s, a);
  const long long nv = a.C * (D / 4);
  hipLaunchKernelGGL(shared_ce_scatter_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, a.dw_part, a.cand, a.dE, a.C, a.rows, D,
                     splits);
  if (a.hs) {
    const long long nh = a.n * (D / 4);
    hipLaunchKernelGGL(shared_ce_scale_rows_kernel<T>, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const T*>(a.h),
                       a.coef_pos, a.mask, a.labels, a.gout, reinterpret_cast<T*>(a.hs), a.tgt, a.n, a.rows, D);
  }
  RG_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int dispatch_fwd(const rg_shared_ce_args& a, int train, hipStream_t s) {
  switch (a.d) {
    case 64: return train ? launch_fwd<T, 64, true>(a, s) : launch_fwd<T, 64, false>(a, s);
    case 128: return train ? launch_fwd<T, 128, true>(a, s) : launch_fwd<T, 128, false>(a, s);
    case 256: return train ? launch_fwd<T, 256, true>(a, s) : launch_fwd<T, 256, false>(a, s);
  }
  return rg_set_error_msg(RG_ERR_UNSUPPORTED, "shared_ce: d must be 64, 128 or 256");
}

template <typename T>
int dispatch_bwd(const rg_shared_ce_args& a, hipStream_t s) {
  switch (a.d) {
    case 64: return launch_bwd<T, 64>(a, s);
    case 128: return launch_bwd<T, 128>(a, s);
    case 256: return launch_bwd<T, 256>(a, s);
  }
  return rg_set_error_msg(RG_ERR_UNSUPPORTED, "shared_ce: d must be 64, 128 or 256");
}

int check_args(const rg_shared_ce_args* a, int dtype, bool fwd, const char* what) {
  static thread_local char msg[200];
  if (!a) return rg_set_error_msg(RG_ERR_INVALID, "shared_ce: args are required");
  if (!(a->d == 64 || a->d == 128 || a->d == 256)) {
    snprintf(msg, sizeof(msg), "%s: d must be 64, 128 or 256 (got %d)", what, a->d);
    return rg_set_error_msg(RG_ERR_UNSUPPORTED, msg);
  }
  if (dtype != RG_BF16 && dtype != RG_X3) {
    snprintf(msg, sizeof(msg), "%s: dtype must be RG_BF16 or RG_X3", what);
    return rg_set_error_msg(RG_ERR_UNSUPPORTED, msg);
  }
  if (a->C < 1 || a->C >= (1LL << 31)) {
    snprintf(msg, sizeof(msg), "%s: C must be in [1, 2^31) (got %lld)", what, a->C);
    return rg_set_error_msg(RG_ERR_INVALID, msg);
  }
  if (a->rows < 1 || a->rows >= (1LL << 31)) {
    snprintf(msg, sizeof(msg), "%s: rows must be in [1, 2^31) (got %lld)", what, a->rows);
    return rg_set_error_msg(RG_ERR_INVALID, msg);
  }
  if (!a->h || (fwd && !a->table) || !a->labels || !a->cand || !a->mask || !a->live16 || !a->wc || !a->lse || !a->sums) {
    snprintf(msg, sizeof(msg), "%s: h,%s labels, cand, mask, live16, wc, lse and sums are required", what, fwd ? " table," : "");
    return rg_set_error_msg(RG_ERR_INVALID, msg);
  }
  return 0;
}

}  // namespace

extern "C" int rg_shared_ce_supported(int d, int dtype) {
  return (d == 64 || d == 128 || d == 256) && (dtype == RG_BF16 || dtype == RG_X3);
}

extern "C" size_t rg_shared_ce_bwd_workspace(long long n, long long C, int d) {
  if (n <= 0 || C < 1 || C >= (1LL << 31) || !(d == 64 || d == 128 || d == 256)) return 0;
  return (size_t)sc_splits(n, C, d) * (size_t)C * (size_t)d * sizeof(float);
}

extern "C" int rg_shared_ce_fwd(const rg_shared_ce_args* a, int train, int dtype, void* stream) {
  if (int e = check_args(a, dtype, true, "shared_ce_fwd")) return e;
  if (a->n <= 0) return 0;
  if (!a->partials || (train && (!a->dh || !a->coef_pos)))
    return rg_set_error_msg(RG_ERR_INVALID, "shared_ce_fwd: partials (and dh, coef_pos for the training form) are required");
  hipStream_t s = (hipStream_t)stream;
  {
    // the candidates index the table and the scatter relies on their being distinct: checked on the host before anything is launched
    // (one copy and a wait on the stream)
    static thread_local char msg[200];
    std::vector<long long> cd((size_t)a->C);
    hipError_t e = hipMemcpyAsync(cd.data(), a->cand, sizeof(long long) * (size_t)a->C, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return rg_set_error(e, __func__);
    for (long long c = 0; c < a->C; ++c) {
      if (cd[c] < 0 || cd[c] >= a->rows) {
        snprintf(msg, sizeof(msg), "shared_ce_fwd: cand[%lld] = %lld is outside the table rows [0, %lld)", c, cd[c], a->rows);
        return rg_set_error_msg(RG_ERR_INVALID, msg);
      }
      if (c > 0 && cd[c] <= cd[c - 1]) {
        snprintf(msg, sizeof(msg), "shared_ce_fwd: cand must be strictly ascending (cand[%lld] = %lld after %lld)", c, cd[c], cd[c - 1]);
        return rg_set_error_msg(RG_ERR_INVALID, msg);
      }
    }
  }
  if (dtype == RG_BF16) return dispatch_fwd<__bf16>(*a, train, s);
  return dispatch_fwd<x3>(*a, train, s);
}

extern "C" int rg_shared_ce_bwd(const rg_shared_ce_args* a, int dtype, void* stream) {
  if (int e = check_args(a, dtype, false, "shared_ce_bwd")) return e;
  if (a->n <= 0) return 0;
  if (!a->dE || !a->dw_part || a->dw_part_bytes < rg_shared_ce_bwd_workspace(a->n, a->C, a->d))
    return rg_set_error_msg(RG_ERR_INVALID, "shared_ce_bwd: dE and dw_part of rg_shared_ce_bwd_workspace() bytes are required");
  if (a->hs && (!a->tgt || !a->coef_pos)) return rg_set_error_msg(RG_ERR_INVALID, "shared_ce_bwd: hs needs tgt and coef_pos");
  if (dtype == RG_BF16) return dispatch_bwd<__bf16>(*a, (hipStream_t)stream);
  return dispatch_bwd<x3>(*a, (hipStream_t)stream);
}

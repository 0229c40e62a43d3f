// Streaming attention core for 416 < L <= 2048 (d_k = d_v = 32): the form behind rg_attn_fwd / rg_attn_bwd for the lengths
// at which one head's key range no longer fits on chip (csrc/attention.hip keeps it resident up to L = 416).
//
// Same contract as the resident kernels (include/recguru_hip.h, rg_attn_args / rg_attn_bwd_args), token-major qkv only:
// scores / sqrt(d_k), REPLACE-fill -1e9 where masked (a fully masked row is uniform over all L keys, quirk Q3), softmax
// in f32, dropout on the probabilities in the attention-map index space ((b*H + h)*L + q) * rg_lpad(L) + key.
//
// Structure: nothing of size L lives in LDS.  A workgroup of four waves owns 64 rows of one (sequence, head) -- 64 queries
// in the forward and in the dQ sweep, 64 keys in the dK / dV sweep -- and walks the other axis in blocks of LK = 64
// positions.  Per block, the one operand that a product needs TRANSPOSED (V^T for O^T = V^T.P^T, Q^T and dO^T for dK / dV,
// K^T for dQ) is staged into a [32][LK + 4] LDS image by all four waves; the row-major operands are 16 / 32-byte fragment
// loads straight from memory (every wave of the workgroup reads the same lines).  The forward keeps a running maximum and
// sum per query (online softmax) and rescales its O^T accumulators when the maximum moves.  Keys of the last, ragged block
// at positions >= L carry NO weight (their probability is set to zero, they never enter the maximum); masked keys are
// finite -1e9 operands of the softmax -- the two are kept apart.
//
// Backward: two launches, no atomics, every output element written by exactly one lane in a fixed order:
// dK / dV by the workgroup that owns the key block (sweeping query blocks), dQ by the one that owns the query block
// (sweeping key blocks).  Both recompute P from lse; the row term is D = dctx . ctx (also under dropout).
//
// Causal: key blocks wholly above the diagonal are not visited -- except for rows whose every visited key was masked
// (the padded prefix of a left-padded sequence): those are uniform over ALL L keys in the reference, so a workgroup that
// holds such a row walks on to the end (the other rows' probabilities there are exp(-1e9 - m) = 0).
//
// Tiers: one template over T = __bf16 / float / x3 -- the products are rg_common.hip.h's mma(): one bf16 MFMA, eight exact
// f32 MFMAs, or the three-MFMA split-operand sum.
#include "rg_common.hip.h"
#include "../../include/recguru_hip.h"

#define DK 32
#define NEG_FILL (-1e9f)
#define NO_KEY (-3.0e38f)     // "no key seen yet" / a position >= L: below every score, finite so that differences stay finite
#define LK 64                 // positions staged per step ("Streaming attention")
#define LDT (LK + 4)          // row pitch of a transposed image: a multiple of 4 (16-byte fragment reads), 8 rows apart = 32 banks

namespace {

struct LongCtx {
  int b, h, blk;              // sequence, head, 64-row block owned by this workgroup
};
__device__ __forceinline__ LongCtx long_ctx(int H, int L) {
  const int nblk = (L + 63) >> 6;
  LongCtx c;
  const int bh = (int)blockIdx.x / nblk;
  c.blk = (int)blockIdx.x - bh * nblk;
  c.b = bh / H;
  c.h = bh - c.b * H;
  return c;
}

// the 16-row tile of positions r0 .. r0 + 15 of sequence b holds a live row (wave-uniform; rowmask == NULL: every row is live)
// rm: this lane's row mask value (row r0 + li; 0 beyond L)
__device__ __forceinline__ bool tile_is_live(const float* __restrict__ rowmask, int b, int L, int r0, int li, float& rm) {
  const int r = r0 + li;
  rm = r < L ? (rowmask ? rowmask[(size_t)b * L + r] : 1.f) : 0.f;
  return __ballot(rm != 0.f) != 0ull;
}

// ------------------------------------------------------------------------------------------------ forward
template <typename T>
__global__ __launch_bounds__(256) void attn_long_fwd_kernel(rg_attn_args a) {
  __shared__ __align__(16) T Vt[DK * LDT];
  __shared__ unsigned char kpad[LK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int L = a.L, H = a.H, P = H * DK, ld = 3 * P;
  const LongCtx c = long_ctx(H, L);
  const int b = c.b, h = c.h;
  const T* __restrict__ qkv = reinterpret_cast<const T*>(a.qkv) + (size_t)b * L * ld;
  T* __restrict__ ctx = reinterpret_cast<T*>(a.ctx) + (size_t)b * L * P + h * DK;
  float* __restrict__ lse = a.lse ? a.lse + ((size_t)b * H + h) * L : nullptr;
  const int q0 = c.blk * 64 + wave * 16, q = q0 + li;
  float rmq;
  const bool live = tile_is_live(a.rowmask, b, L, q0, li, rmq);
  if (!live && q < L) {                       // a skipped tile's rows are WRITTEN: ctx = 0, lse = 0
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    store8(ctx + (size_t)q * P + 8 * lg, z);
    if (lg == 0 && lse) lse[q] = 0.f;
  }
  if (!__syncthreads_or(live ? 1 : 0)) return;

  const DropCfg drop = make_drop(a.drop_p, a.seed);
  const unsigned int dbase = (((unsigned int)b * H + h) * L + (unsigned int)min(q, L - 1)) * rg_lpad(L);
  Frag<T> qf;
  if (live && q < L) load_frag(qf, qkv + (size_t)q * ld + h * DK + 8 * lg);
  else frag_zero(qf);
  float m = NO_KEY, l = 0.f;
  f32x4 o[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
  const int nkb = (L + LK - 1) / LK;
  const int nkb_diag = a.causal ? min(nkb, min(c.blk * 64 + 63, L - 1) / LK + 1) : nkb;

  for (int kb = 0; kb < nkb; ++kb) {
    if (kb == nkb_diag) {                     // past the diagonal: only for rows that have met masked keys alone
      if (!__syncthreads_or((live && q < L && m < -5e8f) ? 1 : 0)) break;
    }
    const int k0 = kb * LK;
    __syncthreads();                          // the previous block's readers are done
    {
      const int row = tid >> 2, c8 = (tid & 3) * 8, key = k0 + row;
      float v[8];
      if (key < L) load8(v, qkv + (size_t)key * ld + 2 * P + h * DK + c8);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) Vt[(c8 + j) * LDT + row] = (T)v[j];
      if ((tid & 3) == 0) kpad[row] = (key < L && a.key_ids[(size_t)b * L + key] == a.pad_value) ? 1 : 0;
    }
    __syncthreads();
    if (!live) continue;                      // (wave-uniform) the wave only helps staging
#pragma unroll
    for (int s = 0; s < LK / 32; ++s) {
      const int ks0 = k0 + 32 * s;
      if (ks0 >= L) break;
      f32x4 sv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int krow = ks0 + u * 16 + li;
        Frag<T> kf;
        if (krow < L) load_frag(kf, qkv + (size_t)krow * ld + P + h * DK + 8 * lg);
        else frag_zero(kf);
        sv[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma(kf, qf, sv[u]);                   // S^T[key][q]
      }
      float sc[2][4];
      float bm = NO_KEY;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = ks0 + u * 16 + 4 * lg + r;
          const bool masked = kpad[key - k0] || (a.causal && key > q);
          const float sval = masked ? NEG_FILL : sv[u][r] * a.scale;
          sc[u][r] = key < L ? sval : NO_KEY;
          bm = fmaxf(bm, sc[u][r]);
        }
      bm = fmaxf(bm, __shfl_xor(bm, 16));
      bm = fmaxf(bm, __shfl_xor(bm, 32));
      const float mn = fmaxf(m, bm);
      const float alpha = __expf(m - mn);
      float k0a[4] = {1.f, 1.f, 1.f, 1.f}, k1a[4] = {1.f, 1.f, 1.f, 1.f};
      if (drop.thresh) rg_keep4_pair(drop, dbase + (unsigned int)(ks0 + 4 * lg), k0a, k1a);
      f32x4 p[2];
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p0 = (ks0 + 4 * lg + r < L) ? __expf(sc[0][r] - mn) : 0.f;
        const float p1 = (ks0 + 16 + 4 * lg + r < L) ? __expf(sc[1][r] - mn) : 0.f;
        ps += p0 + p1;
        p[0][r] = p0 * k0a[r];
        p[1][r] = p1 * k1a[r];
      }
      ps += __shfl_xor(ps, 16);
      ps += __shfl_xor(ps, 32);
      l = l * alpha + ps;
      m = mn;
      Frag<T> pf;
      acc_to_frag(pf, p[0], p[1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
        Frag<T> vtf;
        const T* vp = Vt + (dt * 16 + li) * LDT + 32 * s + 4 * lg;
        load_frag_2x4(vtf, vp, vp + 16);
        mma(vtf, pf, o[dt]);                  // O^T[dv][q] += V^T[dv][key] P^T[key][q]
      }
    }
  }
  if (live && q < L) {
    const float inv = 1.f / l;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const float v4[4] = {o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv};
      store4(ctx + (size_t)q * P + dt * 16 + 4 * lg, v4);
    }
    if (lg == 0 && lse) lse[q] = m + __logf(l);
  }
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
// The workgroup owns keys 64 blk .. 64 blk + 63 (one 16-key tile per wave) and sweeps the query blocks.
template <typename T>
__global__ __launch_bounds__(256) void attn_long_bwd_kv_kernel(rg_attn_bwd_args a) {
  __shared__ __align__(16) T Qt[DK * LDT];
  __shared__ __align__(16) T dOt[DK * LDT];
  __shared__ float lse_s[LK];
  __shared__ float dl_s[LK];
  __shared__ float rm_s[LK];
  __shared__ int live_s[LK / 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int L = a.L, H = a.H, P = H * DK, ld = 3 * P;
  const LongCtx c = long_ctx(H, L);
  const int b = c.b, h = c.h;
  const T* __restrict__ qkv = reinterpret_cast<const T*>(a.qkv) + (size_t)b * L * ld;
  const T* __restrict__ dO = reinterpret_cast<const T*>(a.dctx) + (size_t)b * L * P + h * DK;
  const T* __restrict__ O = reinterpret_cast<const T*>(a.ctx) + (size_t)b * L * P + h * DK;
  const float* __restrict__ lse = a.lse + ((size_t)b * H + h) * L;
  T* __restrict__ dqkv = reinterpret_cast<T*>(a.dqkv) + (size_t)b * L * ld;
  const DropCfg drop = make_drop(a.drop_p, a.seed);
  const unsigned int gbase = ((unsigned int)b * H + h) * L;
  const unsigned int lp = rg_lpad(L);
  const float invL = 1.f / (float)L;

  const int kt0 = c.blk * 64 + wave * 16;
  const int key = kt0 + li;                   // this lane's key (column of S)
  Frag<T> kf, vf;
  if (key < L) {
    load_frag(kf, qkv + (size_t)key * ld + P + h * DK + 8 * lg);
    load_frag(vf, qkv + (size_t)key * ld + 2 * P + h * DK + 8 * lg);
  } else { frag_zero(kf); frag_zero(vf); }
  const bool kmask = key >= L || a.key_ids[(size_t)b * L + min(key, L - 1)] == a.pad_value;
  f32x4 dk[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
  f32x4 dv[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};

  const int nqb = (L + LK - 1) / LK;
  for (int qb = 0; qb < nqb; ++qb) {
    const int qs0 = qb * LK;
    const int row = tid >> 2, c8 = (tid & 3) * 8, qr = qs0 + row;     // wave w stages the 16-query tile w of the block
    float rmr;
    const bool tl = tile_is_live(a.rowmask, b, L, qs0 + wave * 16, row & 15, rmr);
    const bool use = tl && qr < L;
    const float lq = use ? lse[qr] : 0.f;
    // causal: a query block wholly in front of this key block contributes through its fully masked rows alone
    const bool need = use && (!a.causal || qb >= c.blk || lq < -5e8f);
    __syncthreads();                          // the previous block's readers are done
    if (!__syncthreads_or(need ? 1 : 0)) continue;
    {
      float qv[8], gv[8], ov[8];
      if (use) {
        load8(qv, qkv + (size_t)qr * ld + h * DK + c8);
        load8(gv, dO + (size_t)qr * P + c8);
        load8(ov, O + (size_t)qr * P + c8);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { qv[j] = 0.f; gv[j] = 0.f; ov[j] = 0.f; }
      }
      // dctx rows with rowmask == 0 are zero by contract and TAKEN as zero whatever the buffer holds (its producer may leave
      // the rows of padded 16-row tiles of the flattened [B*L] rows unwritten)
      if (rmr == 0.f) {
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] = 0.f;
      }
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        Qt[(c8 + j) * LDT + row] = (T)qv[j];
        dOt[(c8 + j) * LDT + row] = (T)gv[j];
        d += gv[j] * ov[j];
      }
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      if ((tid & 3) == 0) { dl_s[row] = d; lse_s[row] = lq; rm_s[row] = rmr; }
      if (lane == 0) live_s[wave] = tl ? 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < LK / 32; ++s) {
      const bool l0 = live_s[2 * s] != 0, l1 = live_s[2 * s + 1] != 0;
      if (!l0 && !l1) continue;               // (workgroup-uniform) two skipped query tiles
      f32x4 p[2], ds[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        p[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        ds[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (!(u ? l1 : l0)) continue;
        const int qrow = qs0 + s * 32 + u * 16 + li;                  // A-operand row of this lane
        Frag<T> qf, gf;
        if (qrow < L) {
          load_frag(qf, qkv + (size_t)qrow * ld + h * DK + 8 * lg);
          load_frag(gf, dO + (size_t)qrow * P + 8 * lg);
        } else { frag_zero(qf); frag_zero(gf); }
        if (rm_s[s * 32 + u * 16 + li] == 0.f) frag_zero(gf);
        f32x4 sv = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma(qf, kf, sv);                      // S[q][key]
        mma(gf, vf, dp);                      // dP[q][key]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ql = s * 32 + u * 16 + 4 * lg + r, qq = qs0 + ql;   // accumulator row
          const bool masked = kmask || (a.causal && key > qq);
          const float scv = masked ? NEG_FILL : sv[r] * a.scale;
          const float lqq = lse_s[ql];
          // fully masked row: lse = -1e9 + log L rounds to -1e9 in f32, the row is uniform 1/L (Q3)
          const float pv = (qq < L && key < L) ? (lqq < -5e8f ? invL : __expf(scv - lqq)) : 0.f;
          const float ks = drop.thresh ? rg_keep(drop, (gbase + (unsigned int)min(qq, L - 1)) * lp + (unsigned int)key) : 1.f;
          p[u][r] = pv * ks;
          ds[u][r] = masked ? 0.f : pv * (dp[r] * ks - dl_s[ql]) * a.scale;
        }
      }
      Frag<T> pf, dsf;
      acc_to_frag(pf, p[0], p[1]);
      acc_to_frag(dsf, ds[0], ds[1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        Frag<T> gtf, qtf;
        const T* gp = dOt + (dt * 16 + li) * LDT + s * 32 + 4 * lg;
        const T* qp = Qt + (dt * 16 + li) * LDT + s * 32 + 4 * lg;
        load_frag_2x4(gtf, gp, gp + 16);
        load_frag_2x4(qtf, qp, qp + 16);
        mma(pf, gtf, dv[dt]);                 // dV[key][dv] += sum_q P[q][key] dO[q][dv]
        mma(dsf, qtf, dk[dt]);                // dK[key][dk] += sum_q dS[q][key] Q[q][dk]
      }
    }
  }
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int krow = kt0 + 4 * lg + r;
      if (krow < L) {
        dqkv[(size_t)krow * ld + P + h * DK + dt * 16 + li] = (T)dk[dt][r];
        dqkv[(size_t)krow * ld + 2 * P + h * DK + dt * 16 + li] = (T)dv[dt][r];
      }
    }
}

// ------------------------------------------------------------------------------------------------ backward: dQ
// The workgroup owns queries 64 blk .. 64 blk + 63 (one 16-query tile per wave) and sweeps the key blocks.
template <typename T>
__global__ __launch_bounds__(256) void attn_long_bwd_q_kernel(rg_attn_bwd_args a) {
  __shared__ __align__(16) T Kt[DK * LDT];
  __shared__ unsigned char kpad[LK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int L = a.L, H = a.H, P = H * DK, ld = 3 * P;
  const LongCtx c = long_ctx(H, L);
  const int b = c.b, h = c.h;
  const T* __restrict__ qkv = reinterpret_cast<const T*>(a.qkv) + (size_t)b * L * ld;
  const T* __restrict__ dO = reinterpret_cast<const T*>(a.dctx) + (size_t)b * L * P + h * DK;
  const T* __restrict__ O = reinterpret_cast<const T*>(a.ctx) + (size_t)b * L * P + h * DK;
  T* __restrict__ dqkv = reinterpret_cast<T*>(a.dqkv) + (size_t)b * L * ld;
  const int q0 = c.blk * 64 + wave * 16, q = q0 + li;
  float rmq;
  const bool live = tile_is_live(a.rowmask, b, L, q0, li, rmq);
  if (!live && q < L) {                       // dqkv is fully overwritten: the dQ rows of a skipped tile are zeros
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    store8(dqkv + (size_t)q * ld + h * DK + 8 * lg, z);
  }
  if (!__syncthreads_or(live ? 1 : 0)) return;

  const DropCfg drop = make_drop(a.drop_p, a.seed);
  const unsigned int dbase = (((unsigned int)b * H + h) * L + (unsigned int)min(q, L - 1)) * rg_lpad(L);
  Frag<T> qf, gf;
  float lse_q = 0.f, dl_q = 0.f;
  if (live && rmq != 0.f) {                   // (rmq != 0 implies q < L) dctx rows with rowmask == 0 are TAKEN as zero: their dQ row is 0
    load_frag(qf, qkv + (size_t)q * ld + h * DK + 8 * lg);
    load_frag(gf, dO + (size_t)q * P + 8 * lg);
    float gv[8], ov[8];
    load8(gv, dO + (size_t)q * P + 8 * lg);
    load8(ov, O + (size_t)q * P + 8 * lg);
#pragma unroll
    for (int j = 0; j < 8; ++j) dl_q += gv[j] * ov[j];
    lse_q = a.lse[((size_t)b * H + h) * L + q];
  } else { frag_zero(qf); frag_zero(gf); }
  dl_q += __shfl_xor(dl_q, 16);
  dl_q += __shfl_xor(dl_q, 32);
  f32x4 dq[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
  const int nkb = (L + LK - 1) / LK;
  const int nkb_diag = a.causal ? min(nkb, min(c.blk * 64 + 63, L - 1) / LK + 1) : nkb;   // masked scores carry no gradient

  for (int kb = 0; kb < nkb_diag; ++kb) {
    const int k0 = kb * LK;
    __syncthreads();                          // the previous block's readers are done
    {
      const int row = tid >> 2, c8 = (tid & 3) * 8, key = k0 + row;
      float v[8];
      if (key < L) load8(v, qkv + (size_t)key * ld + P + h * DK + c8);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) Kt[(c8 + j) * LDT + row] = (T)v[j];
      if ((tid & 3) == 0) kpad[row] = (key < L && a.key_ids[(size_t)b * L + key] == a.pad_value) ? 1 : 0;
    }
    __syncthreads();
    if (!live) continue;                      // (wave-uniform) the wave only helps staging
#pragma unroll
    for (int s = 0; s < LK / 32; ++s) {
      const int ks0 = k0 + 32 * s;
      if (ks0 >= L) break;
      float k0a[4] = {1.f, 1.f, 1.f, 1.f}, k1a[4] = {1.f, 1.f, 1.f, 1.f};
      if (drop.thresh) rg_keep4_pair(drop, dbase + (unsigned int)(ks0 + 4 * lg), k0a, k1a);
      f32x4 ds[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int krow = ks0 + u * 16 + li;
        Frag<T> kf, vf;
        if (krow < L) {
          load_frag(kf, qkv + (size_t)krow * ld + P + h * DK + 8 * lg);
          load_frag(vf, qkv + (size_t)krow * ld + 2 * P + h * DK + 8 * lg);
        } else { frag_zero(kf); frag_zero(vf); }
        f32x4 sv = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma(kf, qf, sv);                      // S^T[key][q]
        mma(vf, gf, dp);                      // dP^T[key][q]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = ks0 + u * 16 + 4 * lg + r;
          const bool masked = key >= L || kpad[key - k0] || (a.causal && key > q);
          const float pv = (q < L && !masked) ? __expf(sv[r] * a.scale - lse_q) : 0.f;
          const float ks = u ? k1a[r] : k0a[r];
          ds[u][r] = pv * (dp[r] * ks - dl_q) * a.scale;
        }
      }
      Frag<T> dsf;
      acc_to_frag(dsf, ds[0], ds[1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        Frag<T> ktf;
        const T* kp = Kt + (dt * 16 + li) * LDT + 32 * s + 4 * lg;
        load_frag_2x4(ktf, kp, kp + 16);
        mma(ktf, dsf, dq[dt]);                // dQ^T[dk][q] += K^T[dk][key] dS^T[key][q]
      }
    }
  }
  if (live && q < L) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const float v4[4] = {dq[dt][0], dq[dt][1], dq[dt][2], dq[dt][3]};
      store4(dqkv + (size_t)q * ld + h * DK + dt * 16 + 4 * lg, v4);
    }
  }
}

template <typename T>
int launch_long_fwd(const rg_attn_args& a, hipStream_t s) {
  const dim3 grid((unsigned int)(a.B * a.H * ((a.L + 63) / 64))), block(256);
  hipLaunchKernelGGL((attn_long_fwd_kernel<T>), grid, block, 0, s, a);
  RG_CHECK_LAUNCH();
  return 0;
}
template <typename T>
int launch_long_bwd(const rg_attn_bwd_args& a, hipStream_t s) {
  const dim3 grid((unsigned int)(a.B * a.H * ((a.L + 63) / 64))), block(256);
  hipLaunchKernelGGL((attn_long_bwd_kv_kernel<T>), grid, block, 0, s, a);
  RG_CHECK_LAUNCH();
  hipLaunchKernelGGL((attn_long_bwd_q_kernel<T>), grid, block, 0, s, a);
  RG_CHECK_LAUNCH();
  return 0;
}

}   // namespace

// internal to the library: rg_attn_fwd / rg_attn_bwd (attention.hip) hand every L > 416 here
__attribute__((visibility("hidden"))) int rg_attn_long_fwd(const rg_attn_args* a, int dtype, void* stream) {
  if (a->L > 2048) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_fwd: L > 2048 not supported (the streaming form covers 416 < L <= 2048)");
  if (a->x) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_fwd: the x-input form is not supported for L > 416");
  if (a->qkv_hm) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_fwd: head-major qkv (qkv_hm) is not supported for L > 416");
  if (a->x_masked == 2)
    return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_fwd: bias-row substitution (x_masked == 2) is not supported for L > 416");
  if ((long long)a->B * a->H * ((a->L + 63) / 64) > 0x7fffffffll) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_fwd: grid too large");
  if (dtype == RG_BF16) return launch_long_fwd<__bf16>(*a, (hipStream_t)stream);
  if (dtype == RG_F32) return launch_long_fwd<float>(*a, (hipStream_t)stream);
  if (dtype == RG_X3) return launch_long_fwd<x3>(*a, (hipStream_t)stream);
  return rg_set_error_msg(RG_ERR_INVALID, "attn_fwd: bad dtype");
}
__attribute__((visibility("hidden"))) int rg_attn_long_bwd(const rg_attn_bwd_args* a, int dtype, void* stream) {
  if (a->L > 2048) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_bwd: L > 2048 not supported (the streaming form covers 416 < L <= 2048)");
  if (a->qkv_hm) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_bwd: head-major qkv (qkv_hm) is not supported for L > 416");
  if (a->x_masked == 2)
    return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_bwd: bias-row substitution (x_masked == 2) is not supported for L > 416");
  if ((long long)a->B * a->H * ((a->L + 63) / 64) > 0x7fffffffll) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_bwd: grid too large");
  if (dtype == RG_BF16) return launch_long_bwd<__bf16>(*a, (hipStream_t)stream);
  if (dtype == RG_F32) return launch_long_bwd<float>(*a, (hipStream_t)stream);
  if (dtype == RG_X3) return launch_long_bwd<x3>(*a, (hipStream_t)stream);
  return rg_set_error_msg(RG_ERR_INVALID, "attn_bwd: bad dtype");
}

// Attention maps on request (include/recguru_hip.h: rg_attn_probs, rg_attn_cross_probs, rg_attn_rollout): the probability
// matrices the training kernels never store, written to memory for inspection, and their rollout to the input positions.
//
// rg_attn_probs -- softmax(mask(Q K^T * scale)) of every (sequence, head) under rg_attn_args' masking contract: a key is masked
// when key_ids[b, key] == pad_value or (causal and key > q); masked scores are REPLACED by -1e9 (quirk Q3: a row without a
// visible key is uniform over all L keys, future ones included); softmax in f32 over all L keys.
//
// Structure: one streaming form for 1 <= L <= 2048, no LDS at all.  A wave owns 16 query rows of one (b, h) and walks the keys
// 32 at a time, twice: the first sweep keeps a running maximum and sum (online softmax, as attention_long.hip's forward, but
// per LANE over the lane's own keys -- the four lanes of a query are joined once, after the sweep, in a fixed order), the second
// recomputes the scores -- the same instructions on the same operands, so the same bits -- and stores exp(s - m) * (1 / l).
// The K fragments and the key ids of a step are loaded one step ahead of their use; the pad flags of 64 keys are one ballot.
// The product is S^T = K Q^T (keys on the accumulator's rows): a lane then holds FOUR CONSECUTIVE KEYS of
// one query, i.e. 16 contiguous bytes of a map row, and the four lanes of a query cover 64 contiguous bytes per 16-key tile --
// one 16-byte store per lane and tile where the row pitch allows it (L % 4 == 0), four 4-byte stores otherwise.  Every element
// is written by exactly one lane; no atomics.  Keys of the ragged last step (positions >= L) carry no weight and never enter
// the maximum (NO_KEY); masked keys are finite -1e9 operands -- the two are kept apart.
//
// Causal: key steps wholly above the wave's diagonal need no product -- every score there is the fill.  The first sweep stops
// at the diagonal: a row whose maximum is still the fill there has met masked keys alone, so ALL its L scores are the fill and
// its sum is exactly L; for any other row the keys beyond contribute exp(-1e9 - m) = 0.  The second sweep writes them without
// loading K.
//
// Exactness (tests/test_attn_maps_gpu.py): exp(0) = 1 and exp(-1e9 - m) = +0 exactly, the row sum of a one-key row is 1, of a
// row without a visible key L (ones add exactly), and the normaliser is the IEEE quotient 1 / l -- so such rows are exactly
// one-hot / float32(1) / float32(L), and masked keys of any row with a visible key are exactly +0.  The score product and the
// subtraction are kept out of fma contraction so that both sweeps round alike.
//
// Tiers: one template over T = __bf16 / float / x3 on rg_common.hip.h's mma().
#include "rg_common.hip.h"
#include "../../include/recguru_hip.h"
#include <stdio.h>
#include <vector>

#define DK 32
#define NEG_FILL (-1e9f)
#define NO_KEY (-3.0e38f)     // a position >= L / "no key seen yet": below every score, finite so that differences stay finite
#define MAX_L 2048

namespace {

// Scores live in the LOG2 domain: s2 = (q . k) * (scale * log2 e), the fill is -1e9 * log2 e, p = exp2(s2 - m2) -- the softmax is
// the same function, an element costs one multiply less, and exp2(0) = 1 / exp2(fill - m2) = +0 stay exact.
#define LOG2E 1.4426950408889634f
#define FILL2 (NEG_FILL * LOG2E)

// bit r of nib as an all-ones / all-zeros word (v_bfe_i32), and x with `with` substituted where that word is set (v_bfi_b32):
// two VALU operations per element for "masked ? fill : score", no compare, no condition register
__device__ __forceinline__ unsigned int bit_word(unsigned int nib, int r) { return (unsigned int)__builtin_amdgcn_sbfe((int)nib, r, 1); }
__device__ __forceinline__ float subst(unsigned int word, float with, float x) {
  return __uint_as_float((word & __float_as_uint(with)) | (~word & __float_as_uint(x)));
}

struct KeyStep {
  float sc[2][4];             // this lane's 8 scores of a 32-key step: tile u, keys ks0 + 16 u + 4 lg + r of query q (log2 domain)
  unsigned int valid[2];      // (ragged step only) bit r: key ks0 + 16 u + 4 lg + r < L
};

// the pad flags of keys 64 j .. 64 j + 63 as one wave-uniform 64-bit word: each lane compares ONE id (a 512-byte coalesced read)
__device__ __forceinline__ unsigned long long pad_word(int64_t id, int64_t pad_value, int j, int L, int lane) {
  return __ballot(64 * j + lane < L && id == pad_value);
}

// The K operand of a step: rows ks0 + 16 u + li, u = 0, 1.  Loaded ONE STEP AHEAD of its use (a wave's steps are a chain of
// load -> product -> softmax arithmetic; without the prefetch every step waits a full memory round trip).  Rows >= L are read
// from row L - 1 instead (an unconditional load; their scores are replaced by NO_KEY in the ragged step).
template <typename T>
struct KFrags { Frag<T> f[2]; };
template <typename T>
__device__ __forceinline__ void load_k(KFrags<T>& k, const T* __restrict__ kbase, int ld, int ks0, int L, int li) {
#pragma unroll
  for (int u = 0; u < 2; ++u) load_frag(k.f[u], kbase + (size_t)min(ks0 + u * 16 + li, L - 1) * ld);
}
// ... and the ids of 64 keys, one per lane, for pad_word (keys >= L: the id of key L - 1, not counted)
__device__ __forceinline__ int64_t load_id(const int64_t* __restrict__ ids, int j, int L, int lane) { return ids[min(64 * j + lane, L - 1)]; }

// scores of keys ks0 .. ks0 + 31 against the wave's 16 queries.  FULL (wave-uniform): ks0 + 32 <= L, no bounds to watch.
template <typename T, bool FULL>
__device__ __forceinline__ void key_step(KeyStep& k, const rg_attn_probs_args& a, const KFrags<T>& kf, const Frag<T>& qf, unsigned int pad32,
                                         float c, int ks0, int q, int li, int lg) {
  const int L = a.L;
  f32x4 sv[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int u = 0; u < 2; ++u) mma(kf.f[u], qf, sv[u]);       // S^T[key][q]
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int kb = ks0 + u * 16 + 4 * lg;     // this lane's four keys of the tile: kb .. kb + 3
    unsigned int nib = (pad32 >> (u * 16 + 4 * lg)) & 15u;
    if (a.causal) {                           // keys kb + r > q
      const int dq = q - kb;
      nib |= dq >= 3 ? 0u : (dq < 0 ? 15u : ((14u << dq) & 15u));
    }
    unsigned int vn = 15u;
    if (!FULL) {
      const int left = L - kb;                // keys kb + r < L
      vn = left >= 4 ? 15u : (left <= 0 ? 0u : ((1u << left) - 1u));
    }
    k.valid[u] = vn;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = subst(bit_word(nib, r), FILL2, __fmul_rn(sv[u][r], c));
      if (!FULL) s = subst(~bit_word(vn, r), NO_KEY, s);
      k.sc[u][r] = s;
    }
  }
}

// one step of the first sweep: this LANE's running maximum and sum over its own keys (no cross-lane traffic inside the sweep)
template <bool FULL>
__device__ __forceinline__ void lane_online(const KeyStep& k, float& m, float& l) {
  float mn = m;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) mn = fmaxf(mn, k.sc[u][r]);
  float ps = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float e = __builtin_amdgcn_exp2f(__fsub_rn(k.sc[u][r], mn));
      if (!FULL) e = __uint_as_float(__float_as_uint(e) & bit_word(k.valid[u], r));      // a position >= L carries no weight
      ps += e;
    }
  l = l * __builtin_amdgcn_exp2f(__fsub_rn(m, mn)) + ps;
  m = mn;
}

template <typename T>
__global__ __launch_bounds__(256) void attn_probs_kernel(rg_attn_probs_args a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int L = a.L, H = a.H, P = H * DK, ld = 3 * P;
  const int nblk = (L + 63) >> 6;
  const int bh = (int)blockIdx.x / nblk, blk = (int)blockIdx.x - bh * nblk;
  const int b = bh / H, h = bh - b * H;
  const int q0 = blk * 64 + wave * 16, q = q0 + li;
  if (q0 >= L) return;                        // (wave-uniform; the kernel has no barrier)
  const T* __restrict__ qkv = reinterpret_cast<const T*>(a.qkv) + (size_t)b * L * ld;
  const int64_t* __restrict__ ids = a.key_ids + (size_t)b * L;
  const float c = a.scale * LOG2E;
  Frag<T> qf;
  if (q < L) load_frag(qf, qkv + (size_t)q * ld + h * DK + 8 * lg);
  else frag_zero(qf);
  const int nsteps = (L + 31) >> 5, nfull = L >> 5;
  // steps with ks0 <= q0 + 15 hold a key that some query of the wave may see
  const int nsteps_diag = a.causal ? min(nsteps, ((q0 + 15) >> 5) + 1) : nsteps;

  // ---- sweep 1: maximum and sum, per lane over its own keys, joined across the four lanes of a query at the end
  const T* __restrict__ kbase = qkv + P + h * DK + 8 * lg;
  float ml = NO_KEY, ll = 0.f;
  unsigned long long pw = 0ull;
  KFrags<T> kn;
  load_k(kn, kbase, ld, 0, L, li);
  int64_t idn = load_id(ids, 0, L, lane);
  for (int st = 0; st < nsteps_diag; ++st) {
    const KFrags<T> kc = kn;
    if (st + 1 < nsteps_diag) load_k(kn, kbase, ld, (st + 1) * 32, L, li);
    if ((st & 1) == 0) {
      pw = pad_word(idn, a.pad_value, st >> 1, L, lane);
      if (st + 2 < nsteps_diag) idn = load_id(ids, (st >> 1) + 1, L, lane);
    }
    const unsigned int pad32 = (unsigned int)(pw >> (32 * (st & 1)));
    KeyStep k;
    if (st < nfull) {
      key_step<T, true>(k, a, kc, qf, pad32, c, st * 32, q, li, lg);
      lane_online<true>(k, ml, ll);
    } else {
      key_step<T, false>(k, a, kc, qf, pad32, c, st * 32, q, li, lg);
      lane_online<false>(k, ml, ll);
    }
  }
  float m = fmaxf(ml, __shfl_xor(ml, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  float l = ll * __builtin_amdgcn_exp2f(__fsub_rn(ml, m));
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  // (causal) a row that met the fill alone up to its diagonal has L scores, all the fill; for the others the keys beyond add 0
  if (m < -5e8f) l = (float)L;
  const float inv = __fdiv_rn(1.f, l);
  const float pfill = __fmul_rn(__builtin_amdgcn_exp2f(__fsub_rn(FILL2, m)), inv);       // a masked key: +0, or 1 / L in a row of fills

  // ---- sweep 2: recompute and store
  float* __restrict__ row = a.probs + (long long)b * a.b_stride + ((long long)h * L + (long long)min(q, L - 1)) * (long long)L;
  const bool vec4 = ((L & 3) == 0) && ((a.b_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.probs) & 15) == 0);
  load_k(kn, kbase, ld, 0, L, li);
  idn = load_id(ids, 0, L, lane);
  for (int st = 0; st < nsteps; ++st) {
    KeyStep k;
    const bool prod = st < nsteps_diag;         // (wave-uniform) beyond: every key is above the diagonal of every query of the wave
    if (prod) {
      const KFrags<T> kc = kn;
      if (st + 1 < nsteps_diag) load_k(kn, kbase, ld, (st + 1) * 32, L, li);
      if ((st & 1) == 0) {
        pw = pad_word(idn, a.pad_value, st >> 1, L, lane);
        if (st + 2 < nsteps_diag) idn = load_id(ids, (st >> 1) + 1, L, lane);
      }
      const unsigned int pad32 = (unsigned int)(pw >> (32 * (st & 1)));
      if (st < nfull) key_step<T, true>(k, a, kc, qf, pad32, c, st * 32, q, li, lg);
      else key_step<T, false>(k, a, kc, qf, pad32, c, st * 32, q, li, lg);
    }
    if (q >= L) continue;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kb = st * 32 + u * 16 + 4 * lg;
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = prod ? __fmul_rn(__builtin_amdgcn_exp2f(__fsub_rn(k.sc[u][r], m)), inv) : pfill;
      if (vec4) {
        if (kb < L) store4(row + kb, p);      // L % 4 == 0: a group of four keys is whole or absent
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kb + r < L) row[kb + r] = p[r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ cross maps (closed form)
// The decoder-encoder attention sees L copies of one encoder state (quirk Q1): every score of a row is the same number, so the
// row is uniform over the keys with enc_ids != pad_value -- 1 / n_b there, 0 elsewhere, 1 / L everywhere if none is live.
// A (b, h) map is L * L contiguous floats; a workgroup fills CROSS_ROWS rows of it, lanes along the flattened index.
#define CROSS_ROWS 32
__global__ __launch_bounds__(256) void attn_cross_probs_kernel(const int64_t* __restrict__ enc_ids, int64_t pad_value, float* __restrict__ probs,
                                                               long long b_stride, int B, int L, int H) {
  __shared__ int cnt_s[4];
  const int tid = threadIdx.x;
  const int nrb = (L + CROSS_ROWS - 1) / CROSS_ROWS;
  const int bh = (int)blockIdx.x / nrb, rb = (int)blockIdx.x - bh * nrb;
  const int b = bh / H, h = bh - b * H;
  const int64_t* __restrict__ ids = enc_ids + (size_t)b * L;
  int c = 0;
  for (int key = tid; key < L; key += 256) c += ids[key] != pad_value ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((tid & 63) == 0) cnt_s[tid >> 6] = c;
  __syncthreads();
  const int n = cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3];
  const float live_v = __fdiv_rn(1.f, (float)(n > 0 ? n : L));
  const float dead_v = n > 0 ? 0.f : live_v;
  const int r0 = rb * CROSS_ROWS, r1 = min(L, r0 + CROSS_ROWS);
  float* __restrict__ base = probs + (long long)b * b_stride + (long long)h * L * (long long)L;
  const int e1 = r1 * L;                      // L <= 32768: the flattened index of a map fits 31 bits
  for (int e = r0 * L + tid; e < e1; e += 256) {
    const int key = e % L;
    base[e] = ids[key] != pad_value ? live_v : dead_v;
  }
}

// ------------------------------------------------------------------------------------------------ rollout
// r = e_query; for l = N - 1 .. 0: r <- alpha r + (1 - alpha) (r . Abar_l), Abar_l = (1 / H) sum_h maps[b, l, h].
// One workgroup per sequence: r in LDS, thread t owns keys t, t + 256, ... (map rows are read coalesced), queries with r[q] == 0
// are skipped (workgroup-uniform), heads then queries are added in ascending order -- a fixed order, so fixed bits.
#define RO_PER 8              // keys per thread: MAX_L / 256
__global__ __launch_bounds__(256) void attn_rollout_kernel(const float* __restrict__ maps, const int* __restrict__ query, float alpha,
                                                           float* __restrict__ out, int N, int H, int L) {
  __shared__ float r_s[MAX_L];
  const int tid = threadIdx.x, b = (int)blockIdx.x;
  const int qb = query ? query[b] : L - 1;
  for (int key = tid; key < L; key += 256) r_s[key] = key == qb ? 1.f : 0.f;
  __syncthreads();
  const float invH = __fdiv_rn(1.f, (float)H), beta = 1.f - alpha;
  const size_t LL = (size_t)L * L;
  for (int layer = N - 1; layer >= 0; --layer) {
    const float* __restrict__ A = maps + ((size_t)b * N + layer) * H * LL;
    float acc[RO_PER];
#pragma unroll
    for (int j = 0; j < RO_PER; ++j) acc[j] = 0.f;
    for (int q = 0; q < L; ++q) {
      const float rq = r_s[q];
      if (rq == 0.f) continue;
#pragma unroll
      for (int j = 0; j < RO_PER; ++j) {
        const int key = tid + 256 * j;
        if (key < L) {
          float s = 0.f;
          for (int h = 0; h < H; ++h) s += A[h * LL + (size_t)q * L + key];
          acc[j] += rq * (s * invH);
        }
      }
    }
    __syncthreads();                          // every read of r_s of this layer is done
#pragma unroll
    for (int j = 0; j < RO_PER; ++j) {
      const int key = tid + 256 * j;
      if (key < L) r_s[key] = alpha * r_s[key] + beta * acc[j];
    }
    __syncthreads();
  }
  for (int key = tid; key < L; key += 256) out[(size_t)b * L + key] = r_s[key];
}

template <typename T>
int launch_probs(const rg_attn_probs_args& a, hipStream_t s) {
  const dim3 grid((unsigned int)((long long)a.B * a.H * ((a.L + 63) / 64))), block(256);
  hipLaunchKernelGGL((attn_probs_kernel<T>), grid, block, 0, s, a);
  RG_CHECK_LAUNCH();
  return 0;
}

}   // namespace

int rg_attn_probs(const rg_attn_probs_args* a, int dtype, void* stream) {
  if (!a || !a->qkv || !a->key_ids || !a->probs) return rg_set_error_msg(RG_ERR_INVALID, "attn_probs: qkv, key_ids and probs are required");
  if (a->dk != DK) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_probs: d_k must be 32");
  if (a->L > MAX_L) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_probs: L > 2048 not supported");
  if (dtype != RG_BF16 && dtype != RG_F32 && dtype != RG_X3) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_probs: bad dtype");
  if (a->L < 1 || a->H < 1 || a->B < 0) return rg_set_error_msg(RG_ERR_INVALID, "attn_probs: L and H must be >= 1, B >= 0");
  if (a->b_stride < (long long)a->H * a->L * a->L) return rg_set_error_msg(RG_ERR_INVALID, "attn_probs: b_stride < H * L * L");
  if (a->B == 0) return 0;
  if ((long long)a->B * a->H * ((a->L + 63) / 64) > 0x7fffffffll) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_probs: grid too large");
  if (dtype == RG_BF16) return launch_probs<__bf16>(*a, (hipStream_t)stream);
  if (dtype == RG_F32) return launch_probs<float>(*a, (hipStream_t)stream);
  return launch_probs<x3>(*a, (hipStream_t)stream);
}

int rg_attn_cross_probs(const int64_t* enc_ids, int64_t pad_value, float* probs, long long b_stride, int B, int L, int H, void* stream) {
  if (!enc_ids || !probs) return rg_set_error_msg(RG_ERR_INVALID, "attn_cross_probs: enc_ids and probs are required");
  if (L < 1 || H < 1 || B < 0) return rg_set_error_msg(RG_ERR_INVALID, "attn_cross_probs: L and H must be >= 1, B >= 0");
  if (L > 32768) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_cross_probs: L > 32768 not supported");
  if (b_stride < (long long)H * L * L) return rg_set_error_msg(RG_ERR_INVALID, "attn_cross_probs: b_stride < H * L * L");
  if (B == 0) return 0;
  const long long nwg = (long long)B * H * ((L + CROSS_ROWS - 1) / CROSS_ROWS);
  if (nwg > 0x7fffffffll) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_cross_probs: grid too large");
  hipLaunchKernelGGL(attn_cross_probs_kernel, dim3((unsigned int)nwg), dim3(256), 0, (hipStream_t)stream, enc_ids, pad_value, probs, b_stride,
                     B, L, H);
  RG_CHECK_LAUNCH();
  return 0;
}

int rg_attn_rollout(const float* maps, const int* query, float alpha, float* out, int B, int N, int H, int L, void* stream) {
  static thread_local char msg[160];
  if (!maps || !out) return rg_set_error_msg(RG_ERR_INVALID, "attn_rollout: maps and out are required");
  if (N < 1 || H < 1 || L < 1 || B < 0) return rg_set_error_msg(RG_ERR_INVALID, "attn_rollout: N, H and L must be >= 1, B >= 0");
  if (L > MAX_L) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "attn_rollout: L > 2048 not supported");
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (query) {
    // the queries index the map rows: checked on the host before anything is launched (one small copy and a wait on the stream)
    std::vector<int> qh((size_t)B);
    hipError_t e = hipMemcpyAsync(qh.data(), query, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return rg_set_error(e, __func__);
    for (int b = 0; b < B; ++b)
      if (qh[b] < 0 || qh[b] >= L) {
        snprintf(msg, sizeof(msg), "attn_rollout: query[%d] = %d is outside the positions [0, %d)", b, qh[b], L);
        return rg_set_error_msg(RG_ERR_INVALID, msg);
      }
  }
  hipLaunchKernelGGL(attn_rollout_kernel, dim3((unsigned int)B), dim3(256), 0, s, maps, query, alpha, out, N, H, L);
  RG_CHECK_LAUNCH();
  return 0;
}

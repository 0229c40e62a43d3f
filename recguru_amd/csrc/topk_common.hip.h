// What csrc/topk.hip and csrc/topk_wide.hip share: the score function, the 64-bit key, the row / user loads of the catalogue walk, the
// exclusion-run search, the list helpers and the slicing of the catalogue.  ONE tk_scores() and ONE key layout for every top-K entry
// point: equal (user, row) pairs give equal bits in rg_topk_scores, rg_topk_list and rg_topk_wide.  Everything is internal to the
// including unit (anonymous namespace); no float atomics, no rg_det.hip.h.
#pragma once
#include "rg_common.hip.h"

namespace {

constexpr int TK_WAVES = 4;
constexpr int TK_THREADS = TK_WAVES * RG_WAVE;
constexpr int TK_UB = TK_WAVES * 16;        // users per workgroup
constexpr int TK_MAX_SLICES = 64;
constexpr int TK_TARGET_WGS = 1024;
constexpr int TK_MAX_K = 128;
constexpr int TK_MERGE_THREADS = 256;

typedef unsigned long long tk_key;          // (order-preserving image of the score) << 32 | (0xFFFFFFFF - row in the catalogue); 0 = empty

__device__ __forceinline__ tk_key tk_make_key(float s, unsigned int row) {
  const unsigned int u = __float_as_uint(s + 0.f);          // -0 -> +0: equal scores, equal images
  const unsigned int o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((tk_key)o << 32) | (tk_key)(0xFFFFFFFFu - row);
}
__device__ __forceinline__ float tk_key_score(tk_key k) {
  const unsigned int o = (unsigned int)(k >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ unsigned int tk_key_row(tk_key k) { return 0xFFFFFFFFu - (unsigned int)k; }

__device__ __forceinline__ tk_key tk_readlane(tk_key v, int l) {
  const unsigned int lo = __builtin_amdgcn_readlane((int)(unsigned int)v, l), hi = __builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), l);
  return ((tk_key)hi << 32) | lo;
}
__device__ __forceinline__ tk_key tk_shfl_xor(tk_key v, int o) {
  const unsigned int lo = __shfl_xor((int)(unsigned int)v, o), hi = __shfl_xor((int)(unsigned int)(v >> 32), o);
  return ((tk_key)hi << 32) | lo;
}

// raw fragment (as loaded) -> MFMA operand: the bf16 tier's is the fragment, the x3 tier's the split pair
__device__ __forceinline__ void tk_to_op(Frag<__bf16>& o, const Frag<__bf16>& r) { o = r; }
__device__ __forceinline__ void tk_to_op(FragX3& o, const Frag<x3>& r) { split_x3(r.v, o.hi, o.lo); }

// the score tile: acc reg r of lane (g, i) = A row 4 g + r (a user) . B column i (a catalogue row)
template <typename T, int KS>
__device__ __forceinline__ f32x4 tk_scores(const typename OpT<T>::type (&a)[KS], const Frag<T> (&braw)[KS]) {
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    typename OpT<T>::type b;
    tk_to_op(b, braw[ks]);
    mma(a[ks], b, acc);
  }
  return acc;
}

// row `row` of src (row < 0: zeros) as the lane's share of KS k-steps
template <typename T, int D>
__device__ __forceinline__ void tk_load_row(Frag<T> (&f)[D / 32], const T* __restrict__ src, long long row, int g) {
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    if (row >= 0) load_frag(f[ks], src + row * D + ks * 32 + 8 * g);
    else frag_zero(f[ks]);
  }
}

// the wave's 16 users as A operands
template <typename T, int D>
__device__ __forceinline__ void tk_load_users(typename OpT<T>::type (&ha)[D / 32], const T* __restrict__ H, long long b, int B, int g) {
  Frag<T> raw[D / 32];
  tk_load_row<T, D>(raw, H, b < B ? b : -1, g);
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) tk_to_op(ha[ks], raw[ks]);
}

// id in the sorted run ex[lo, hi)?
__device__ __forceinline__ bool tk_excluded(const int64_t* __restrict__ ex, long long lo, long long hi, long long id) {
  const long long end = hi;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (ex[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && ex[lo] == id;
}

// one key into user list lst[0, K): nothing if it does not beat the worst kept key, else it replaces it (wave-uniform arguments)
__device__ __forceinline__ void tk_insert(volatile tk_key* lst, int K, volatile tk_key* thr, volatile int* wpos, tk_key ck, int lane) {
  if (ck <= *thr) return;
  const int p = *wpos;
  if (lane == 0) lst[p] = ck;
  __builtin_amdgcn_wave_barrier();
  tk_key w = ~0ull;
  int wp = 0;
  for (int e = lane; e < K; e += RG_WAVE) {
    const tk_key v = lst[e];
    if (v < w) { w = v; wp = e; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const tk_key ow = tk_shfl_xor(w, o);
    const int op = __shfl_xor(wp, o);
    if (ow < w || (ow == w && op < wp)) { w = ow; wp = op; }
  }
  if (lane == 0) { *thr = w; *wpos = wp; }
  __builtin_amdgcn_wave_barrier();
}

// table row at position pos of the list (-1 past its end)
__device__ __forceinline__ int tk_list_id(const int64_t* __restrict__ rows, unsigned int pos, unsigned int n) {
  return pos < n ? (int)rows[pos] : -1;                         // (table_rows < 2^31: one register)
}

// the first position p of rows that is outside [0, table_rows) or not above rows[p - 1] -> *bad (preset to ~0): the body of the
// check kernel of either unit; the kernel passes its own first position and grid stride
__device__ __forceinline__ void tk_list_check(const int64_t* __restrict__ rows, long long n, long long table_rows,
                                              unsigned long long* __restrict__ bad, long long p0, long long step) {
  for (long long p = p0; p < n; p += step) {
    const long long v = rows[p];
    if (v < 0 || v >= table_rows || (p > 0 && v <= (long long)rows[p - 1])) atomicMin(bad, (unsigned long long)p);
  }
}

// catalogue slices of the walk: enough workgroups to fill the device, whatever n_rows
inline int tk_slices(int B) {
  const int nub = (B + TK_UB - 1) / TK_UB;
  const int s = (TK_TARGET_WGS + nub - 1) / nub;
  return s < 1 ? 1 : (s > TK_MAX_SLICES ? TK_MAX_SLICES : s);
}

}  // namespace

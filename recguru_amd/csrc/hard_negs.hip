// Hard negatives: per live position the skip .. skip + k - 1 best ids of ONE sampled pool, the position's own label and its sequence's
// exclusion row left out (include/recguru_hip.h, rg_hard_negs).  The training form of the list walk of topk.hip:
//
//   score(t, c) = h[t] . table[pool[c]] -- tk_scores(), the ONE score function of the top-K units: a 16 x 16 MFMA tile, positions as
//   the A rows, pool rows as the B columns, the k-steps in ascending order.  An output element is a function of its A row and its B
//   column only, so a (h row, table row) pair has the bits it has in rg_topk_scores / rg_topk_list, whatever n, L, the tile or the pool.
//
// hn_kernel: one wave per LIVE 16-position tile (rg_live_tiles; the grid covers every tile, a wave past the live count leaves at once --
// the count stays on the device), 4 waves per workgroup, no workgroup barrier.  The tile's h rows sit in registers as presplit A
// operands; the pool is walked in 16-row tiles, the dependent load (id, then row) pipelined two deep as in the LIST form of
// tk_main_kernel.  Each position keeps its skip + k best keys in LDS owned by its wave (threshold compare, tk_insert: replace the worst,
// rescan).  A key that passes the threshold is then tested against the label and the sequence's exclusion row (binary search) -- few
// keys once the lists have warmed up.  The key packs the POSITION in the pool (an ascending pool keeps "lower id first" for ties) and is
// decoded through pool at the end, where the wave ranks each of its 16 lists by counting and writes ranks skip .. skip + k - 1; a slot
// the position has no id for is not written.  One pass, one launch; nothing of size [n, C]; no float atomics, no rg_det.hip.h.
//
// A pool id outside [0, table_rows) is never dereferenced: hn_pool_id turns it into -1, the column scores a zero row and is ineligible.
// checked = 0 runs tk_list_check first (the one word is allocated by the call, copied back and waited for).
#include "rg_common.hip.h"
#include "topk_common.hip.h"          // tk_scores(), the key, the row / user loads, tk_excluded, tk_insert, tk_list_check
#include "../../include/recguru_hip.h"

namespace {

// table row at position pos of the pool; -1 past its end or outside the table
__device__ __forceinline__ int hn_pool_id(const int64_t* __restrict__ pool, unsigned int pos, unsigned int C, long long table_rows) {
  if (pos >= C) return -1;
  const long long v = pool[pos];
  return (v >= 0 && v < table_rows) ? (int)v : -1;               // (table_rows < 2^31: one register)
}

template <typename T, int D>
__global__ __launch_bounds__(TK_THREADS) void hn_kernel(rg_hard_negs_args a) {
  extern __shared__ __align__(16) unsigned char hn_lds[];
  __shared__ tk_key thr_s[TK_WAVES][16];
  __shared__ int wpos_s[TK_WAVES][16];
  constexpr int KS = D / 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const int e = (int)blockIdx.x * TK_WAVES + wave;
  if (e >= a.live16[0]) return;                                  // (no workgroup barrier below: the waves are independent)
  const long long t0 = (long long)a.live16[1 + e] * 16;
  const int K = a.skip + a.k;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.table);
  tk_key* list_nv = reinterpret_cast<tk_key*>(hn_lds) + (size_t)wave * 16 * K;          // [16][K]
  volatile tk_key* list = list_nv;
  volatile tk_key* thr = thr_s[wave];
  volatile int* wpos = wpos_s[wave];
  for (int q = lane; q < 16 * K; q += RG_WAVE) list[q] = 0;
  if (lane < 16) { thr[lane] = 0; wpos[lane] = 0; }
  __builtin_amdgcn_wave_barrier();

  typename OpT<T>::type ha[KS];
  tk_load_users<T, D>(ha, H, t0 + i, (int)a.n, g);
  // the lane's four positions 4 g + r
  bool uv[4];
  int lab[4];
  long long e0[4], e1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long t = t0 + 4 * g + r;
    uv[r] = t < a.n && a.mask[t] != 0.f;
    const long long y = uv[r] ? (long long)a.labels[t] : -1;
    lab[r] = (y >= 0 && y < a.table_rows) ? (int)y : -1;         // (a label outside the table equals no pool id)
    const long long b = t / a.L;
    e0[r] = (a.excl && uv[r]) ? a.excl_lo[b] : 0;
    e1[r] = (a.excl && uv[r]) ? a.excl_hi[b] : 0;
  }

  const unsigned int C = (unsigned int)a.C;
  const long long ntiles = (a.C + 15) / 16;
  Frag<T> cur[KS], nxt[KS];
  // the table row of column i: of the tile being scored, and of the tile whose fragments are fetched next
  int id_cur = hn_pool_id(a.pool, (unsigned int)i, C, a.table_rows), id_nxt = -1;
  tk_load_row<T, D>(cur, W, id_cur, g);
  if (1 < ntiles) id_nxt = hn_pool_id(a.pool, 16u + (unsigned int)i, C, a.table_rows);
  for (long long tile = 0; tile < ntiles; ++tile) {
    const unsigned int pos = (unsigned int)(tile * 16 + i);      // position in the pool (< 2^31)
    int id_after = -1;
    if (tile + 1 < ntiles) {
      tk_load_row<T, D>(nxt, W, id_nxt, g);
      if (tile + 2 < ntiles) id_after = hn_pool_id(a.pool, pos + 32u, C, a.table_rows);
    }
    const f32x4 acc = tk_scores<T, KS>(ha, cur);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const tk_key key = tk_make_key(acc[r], pos);
      bool pass = id_cur >= 0 && uv[r] && key > thr[4 * g + r];
      if (pass) pass = id_cur != lab[r] && !tk_excluded(a.excl, e0[r], e1[r], (long long)id_cur);          // (no row: e0 == e1, excl is not read)
      unsigned long long m = __ballot(pass);
      while (m) {
        const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
        m &= m - 1;
        const int u = 4 * (l >> 4) + r;
        tk_insert(list + u * K, K, thr + u, wpos + u, tk_readlane(key, l), lane);
      }
    }
    if (tile + 1 < ntiles) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) cur[ks] = nxt[ks];
    }
    id_cur = id_nxt;
    id_nxt = id_after;
  }
  __builtin_amdgcn_wave_barrier();

  // each list ranked by counting (its keys are distinct): the key with rho keys above it is the rho-th of the order
  for (int u = 0; u < 16; ++u) {
    const long long t = t0 + u;
    if (t >= a.n || a.mask[t] == 0.f) continue;                  // (wave-uniform)
    const tk_key* lst = list_nv + u * K;
    int cnt = 0;
    for (int q0 = 0; q0 < K; q0 += RG_WAVE) {
      const int q = q0 + lane;
      const tk_key mine = q < K ? lst[q] : 0;
      int rho = 0;
      cnt = 0;
#pragma unroll 8
      for (int p = 0; p < K; ++p) {
        const tk_key v = lst[p];
        rho += v > mine ? 1 : 0;
        cnt += v != 0 ? 1 : 0;
      }
      const int j = rho - a.skip;
      if (mine != 0 && j >= 0) {                                 // (j < k: rho < K)
        a.out[t * a.ld_out + j] = a.pool[tk_key_row(mine)];
        if (a.out_scores) a.out_scores[t * a.k + j] = tk_key_score(mine);
      }
    }
    if (a.out_scores)
      for (int j = lane; j < a.k; j += RG_WAVE)
        if (a.skip + j >= cnt) a.out_scores[t * a.k + j] = -INFINITY;
  }
}

__global__ __launch_bounds__(256) void hn_check_kernel(const int64_t* __restrict__ pool, long long n, long long table_rows,
                                                       unsigned long long* __restrict__ bad) {
  const long long step = (long long)gridDim.x * blockDim.x;
  tk_list_check(pool, n, table_rows, bad, (long long)blockIdx.x * blockDim.x + threadIdx.x, step);
}

template <typename T, int D>
int hn_launch(const rg_hard_negs_args& a, hipStream_t s) {
  const long long nt = (a.n + 15) / 16;
  const size_t lds = (size_t)TK_WAVES * 16 * (size_t)(a.skip + a.k) * sizeof(tk_key);
  auto k = hn_kernel<T, D>;
  hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, dim3((unsigned int)((nt + TK_WAVES - 1) / TK_WAVES)), dim3(TK_THREADS), lds, s, a);
  RG_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int hn_dispatch(const rg_hard_negs_args& a, hipStream_t s) {
  switch (a.d) {
    case 64: return hn_launch<T, 64>(a, s);
    case 128: return hn_launch<T, 128>(a, s);
    case 256: return hn_launch<T, 256>(a, s);
  }
  return rg_set_error_msg(RG_ERR_UNSUPPORTED, "hard_negs: d must be 64, 128 or 256");
}

// the device-side check of the pool: 0 = fine, else the refusal (already recorded)
int hn_check_pool(const rg_hard_negs_args& a, hipStream_t s) {
  static thread_local char msg[200];
  unsigned long long* bad_d = nullptr;
  unsigned long long bad = 0;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&bad_d), sizeof(bad));
  if (e != hipSuccess) return rg_set_error(e, __func__);
  long long v[2] = {0, 0};
  e = hipMemsetAsync(bad_d, 0xFF, sizeof(bad), s);
  if (e == hipSuccess) {
    const long long blocks = (a.C + 255) / 256;
    hipLaunchKernelGGL(hn_check_kernel, dim3((unsigned int)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, a.pool, a.C, a.table_rows, bad_d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, bad_d, sizeof(bad), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  const long long p = (long long)bad;
  if (e == hipSuccess && bad != ~0ull) {
    // the refusal's message wants the offending value and its predecessor: two more words, on this path only
    e = hipMemcpyAsync(v, a.pool + (p > 0 ? p - 1 : 0), sizeof(long long) * (p > 0 ? 2 : 1), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  hipFree(bad_d);
  if (e != hipSuccess) return rg_set_error(e, __func__);
  if (bad == ~0ull) return 0;
  const long long cur = p > 0 ? v[1] : v[0];
  if (cur < 0 || cur >= a.table_rows)
    snprintf(msg, sizeof(msg), "hard_negs: pool[%lld] = %lld is outside the table rows [0, %lld)", p, cur, a.table_rows);
  else
    snprintf(msg, sizeof(msg), "hard_negs: pool must be strictly ascending (pool[%lld] = %lld after %lld)", p, cur, v[0]);
  return rg_set_error_msg(RG_ERR_INVALID, msg);
}

}  // namespace

extern "C" int rg_hard_negs(const rg_hard_negs_args* a, int dtype, void* stream) {
  if (!a) return rg_set_error_msg(RG_ERR_INVALID, "hard_negs: args are required");
  if (dtype != RG_BF16 && dtype != RG_X3) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "hard_negs: dtype must be RG_BF16 or RG_X3");
  if (a->d != 64 && a->d != 128 && a->d != 256) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "hard_negs: d must be 64, 128 or 256");
  if (a->k < 1) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "hard_negs: k must be at least 1");
  if (a->skip < 0) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "hard_negs: skip must not be negative");
  if ((long long)a->skip + a->k > TK_MAX_K) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "hard_negs: skip + k must be at most 128");
  if (a->C < 1 || a->C >= (1LL << 31)) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "hard_negs: C must be in [1, 2^31)");
  if (a->table_rows < 1 || a->table_rows >= (1LL << 31)) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "hard_negs: table_rows must be in [1, 2^31)");
  if (a->n < 0 || a->n >= (1LL << 31)) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "hard_negs: n must be in [0, 2^31)");
  if (a->L < 1) return rg_set_error_msg(RG_ERR_INVALID, "hard_negs: L must be at least 1");
  if (a->n % a->L != 0) return rg_set_error_msg(RG_ERR_INVALID, "hard_negs: n must be a multiple of L");
  if (a->ld_out < a->k) return rg_set_error_msg(RG_ERR_INVALID, "hard_negs: ld_out must be at least k");
  if (a->n == 0) return 0;
  if (!a->h || !a->table || !a->pool || !a->labels || !a->mask || !a->live16 || !a->out)
    return rg_set_error_msg(RG_ERR_INVALID, "hard_negs: h, table, pool, labels, mask, live16 and out are required");
  if (a->excl && (!a->excl_lo || !a->excl_hi)) return rg_set_error_msg(RG_ERR_INVALID, "hard_negs: excl needs excl_lo and excl_hi");
  hipStream_t s = (hipStream_t)stream;
  if (!a->checked) {
    const int rc = hn_check_pool(*a, s);
    if (rc) return rc;
  }
  if (dtype == RG_BF16) return hn_dispatch<__bf16>(*a, s);
  return hn_dispatch<x3>(*a, s);
}

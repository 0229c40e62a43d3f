// Full-catalogue scoring without the score matrix: per user the K best catalogue rows of h @ table.T and the exact rank of a target
// among all of them (the inference-side counterpart of full_ce.hip; include/recguru_hip.h, rg_topk_scores).
//
//   score(b, i) = h[b] . table[i]   -- ONE function, tk_scores(): a 16 x 16 MFMA tile, users as the A rows, catalogue rows as the B
//   columns, the k-steps in ascending order.  An output element of the MFMA is a function of its A row and its B column only, so a
//   score does not depend on the tile, the workgroup, the slice or B that produced it: equal pairs give equal bits, and the top-K
//   of per-slice top-Ks is the global top-K under one total order.
//
// Three kernels, no float atomics (deterministic in both libraries; this unit does not include rg_det.hip.h):
//   tk_gather_kernel   (target given) one wave per 16 users: the score of (b, target[b]) -> tscore[b], and the number of row b's
//       exclusion ids (other than the target, inside the catalogue) that score strictly higher -> rank[b] = -that.  A gathered row
//       goes through tk_scores() as column i of a tile whose diagonal is read.
//   tk_main_kernel     grid (user blocks of 64, slices).  A wave owns 16 users (h as presplit A operands in registers) and walks the
//       16-row tiles of its slice, the next tile's rows prefetched into registers.  Per tile: rank[b] += #(score > tscore[b]) (the
//       target itself scores tscore[b] exactly, excluded ids were subtracted by the gather kernel), and every score packed with its
//       row into a 64-bit key (score order, then lower row first) is compared with the user's threshold = the worst of its K kept
//       keys (LDS, owned by the wave: no barrier in the loop).  Keys that pass -- few once the list has warmed up -- are looked up
//       in the exclusion row (binary search) and inserted one by one: replace the worst, rescan for the new worst (wave-wide).  The
//       kept set is the K best keys of the slice whatever the insertion order.  Each (slice, user) writes its K keys to the workspace.
//   tk_merge_kernel    one workgroup per user: bitonic sort of the slices' keys in LDS, the first K decoded to (id, score).
//
// Workspace: align256(4 B) + S B K 8 bytes, S = tk_slices(B) = clamp(ceil(1024 / ceil(B / 64)), 1, 64) -- independent of n_rows.
//
// Candidate lists (rg_topk_list): the same three kernels instantiated with LIST = true walk rows[0, n_list), an ascending list of table
// rows shared by the batch, instead of a row range; LIST = false is the range walk, line for line what it was.  The "catalogue" of the
// list form is the POSITIONS 0 .. n_list - 1 (first_row = 0, n_rows = n_list in the kernels' rg_topk_args): slices are ranges of list
// tiles, keys pack the position (an ascending list keeps "lower id first" for ties), tk_merge_kernel decodes through rows.  The walk's
// dependent load (id, then row) is pipelined two deep: while a tile is scored the next tile's row fragments are in flight and so is
// the id of the tile after that -- one register per lane, so that the list form keeps the range form's waves per SIMD where
// the range form sits just under a step (124 VGPRs at bf16 d = 128).  tk_gather_kernel scores the target
// wherever it sits in the table and counts an exclusion id only when a binary search finds it in rows.  tk_list_check_kernel leaves
// the first position of rows that is out of the table or not above its predecessor in one word (integer atomicMin), read back with
// the wait the call does anyway; the workspace holds that word (256 bytes) after tscore.
#include <vector>

#include "rg_common.hip.h"
#include "topk_common.hip.h"          // tk_scores(), the key, the row / user loads, tk_excluded, tk_insert, the list helpers, tk_slices: shared with topk_wide.hip and hard_negs.hip
#include "../../include/recguru_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------
// target scores and the exclusion rows' share of the rank
// ------------------------------------------------------------------------------------------------
// LIST: rows[0, a.n_rows) is the candidate list (a.first_row = 0), targets are rows of the table [0, table_rows)
template <typename T, int D, bool LIST>
__global__ __launch_bounds__(TK_THREADS) void tk_gather_kernel(rg_topk_args a, const int64_t* __restrict__ rows, long long table_rows,
                                                               float* __restrict__ tscore) {
  constexpr int KS = D / 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const long long ub0 = ((long long)blockIdx.x * TK_WAVES + wave) * 16;
  if (ub0 >= a.B) return;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.table);
  typename OpT<T>::type ha[KS];
  tk_load_users<T, D>(ha, H, ub0 + i, a.B, g);

  // column i of every tile belongs to user ub0 + i
  const long long b = ub0 + i;
  const bool bv = b < a.B;
  const long long row_end = a.first_row + a.n_rows;
  long long tgt = bv ? (long long)a.target[b] : -1;
  if (LIST ? (tgt < 0 || tgt >= table_rows) : (tgt < a.first_row || tgt >= row_end)) tgt = -1;          // (the host has refused such a call: never outside the table)
  long long e0 = 0, len = 0;
  if (bv && a.excl) {
    e0 = a.excl_off[b];
    len = a.excl_off[b + 1] - e0;
  }
  long long maxlen = len;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const long long other = __shfl_xor(maxlen, o);
    maxlen = other > maxlen ? other : maxlen;
  }
  float t = 0.f;
  int higher = 0;
  for (long long j = 0; j <= maxlen; ++j) {
    long long id = -1;
    if (j == 0) id = tgt;
    else if (j - 1 < len) {
      id = a.excl[e0 + j - 1];
      if (LIST) {
        if (id == tgt || !tk_excluded(rows, 0, a.n_rows, id)) id = -1;          // not a member of the list (or outside the table): no share
      } else if (id == tgt || id < a.first_row || id >= row_end) id = -1;
    }
    Frag<T> wb[KS];
    tk_load_row<T, D>(wb, W, id, g);
    const f32x4 acc = tk_scores<T, KS>(ha, wb);
    // the diagonal element sits in lane (i >> 2, i), reg i & 3: picked with masks (a select chain becomes a jump table whose
    // accumulator copies sit in front of exec restores -- the build's ISA screen refuses that shape)
    unsigned int sb = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) sb |= __float_as_uint(acc[r]) & (0u - (unsigned int)((i & 3) == r));
    const float s = __uint_as_float(sb);
    if (j == 0) t = s;
    else if (id >= 0 && s > t) ++higher;
  }
  if (bv && g == (i >> 2)) {
    tscore[b] = t;
    a.rank[b] = -higher;
  }
}

// ------------------------------------------------------------------------------------------------
// the pass over the catalogue
// ------------------------------------------------------------------------------------------------
template <typename T, int D, bool LIST>
__global__ __launch_bounds__(TK_THREADS) void tk_main_kernel(rg_topk_args a, const int64_t* __restrict__ rows, const float* __restrict__ tscore,
                                                             tk_key* __restrict__ part, long long tiles_per_slice) {
  extern __shared__ __align__(16) unsigned char tk_lds[];
  __shared__ tk_key thr_s[TK_WAVES][16];
  __shared__ int wpos_s[TK_WAVES][16];
  constexpr int KS = D / 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const int K = a.K;
  const long long ub0 = ((long long)blockIdx.x * TK_WAVES + wave) * 16;
  if (ub0 >= a.B) return;                                      // (no workgroup barrier below: the waves are independent)
  const int slice = blockIdx.y;
  const bool want_rank = a.rank != nullptr;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.table) + a.first_row * D;
  volatile tk_key* list = reinterpret_cast<tk_key*>(tk_lds) + (size_t)wave * 16 * K;        // [16][K]
  volatile tk_key* thr = thr_s[wave];
  volatile int* wpos = wpos_s[wave];
  for (int e = lane; e < 16 * K; e += RG_WAVE) list[e] = 0;
  if (lane < 16) { thr[lane] = 0; wpos[lane] = 0; }
  __builtin_amdgcn_wave_barrier();

  typename OpT<T>::type ha[KS];
  tk_load_users<T, D>(ha, H, ub0 + i, a.B, g);
  // the lane's four users 4 g + r
  bool uv[4];
  float t[4];
  long long e0[4], e1[4];
  int cnt[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long b = ub0 + 4 * g + r;
    uv[r] = b < a.B;
    t[r] = (want_rank && uv[r]) ? tscore[b] : INFINITY;
    e0[r] = (a.excl && uv[r]) ? a.excl_off[b] : 0;
    e1[r] = (a.excl && uv[r]) ? a.excl_off[b + 1] : 0;
    cnt[r] = 0;
  }

  const long long ntiles = (a.n_rows + 15) / 16;
  const long long tile0 = (long long)slice * tiles_per_slice;
  const long long tile1 = tile0 + tiles_per_slice < ntiles ? tile0 + tiles_per_slice : ntiles;
  Frag<T> cur[KS], nxt[KS];
  // LIST: the table row of column i in the tile whose fragments are fetched next -- one register: once those loads are issued it
  // takes the id of the tile after (in flight during this tile's MFMAs); the exclusion search, rare, reads its id again
  int id_nxt = -1;
  const unsigned int n_list = (unsigned int)a.n_rows;
  if (tile0 < tile1) {
    const long long row = tile0 * 16 + i;
    if (LIST) {
      tk_load_row<T, D>(cur, W, tk_list_id(rows, (unsigned int)row, n_list), g);
      if (tile0 + 1 < tile1) id_nxt = tk_list_id(rows, (unsigned int)row + 16, n_list);
    } else {
      tk_load_row<T, D>(cur, W, row < a.n_rows ? row : -1, g);
    }
  }
  for (long long tile = tile0; tile < tile1; ++tile) {
    if (tile + 1 < tile1) {
      const long long row = (tile + 1) * 16 + i;
      if (LIST) {
        tk_load_row<T, D>(nxt, W, id_nxt, g);
        if (tile + 2 < tile1) id_nxt = tk_list_id(rows, (unsigned int)row + 16, n_list);
      } else {
        tk_load_row<T, D>(nxt, W, row < a.n_rows ? row : -1, g);
      }
    }
    const f32x4 acc = tk_scores<T, KS>(ha, cur);
    const long long row = tile * 16 + i;                       // row in the catalogue (< 2^31); LIST: position in the list
    const bool iv = row < a.n_rows;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = acc[r];
      cnt[r] += (iv && s > t[r]) ? 1 : 0;                       // t = +inf: no rank wanted / no such user
      if (K > 0) {
        const tk_key key = tk_make_key(s, (unsigned int)row);
        bool pass = iv && uv[r] && key > thr[4 * g + r];
        if (pass && a.excl) pass = !tk_excluded(a.excl, e0[r], e1[r], LIST ? (long long)rows[(unsigned int)row] : a.first_row + row);
        unsigned long long m = __ballot(pass);
        while (m) {
          const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
          m &= m - 1;
          const int u = 4 * (l >> 4) + r;
          tk_insert(list + u * K, K, thr + u, wpos + u, tk_readlane(key, l), lane);
        }
      }
    }
    if (tile + 1 < tile1) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) cur[ks] = nxt[ks];
    }
  }

  if (want_rank) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int c = cnt[r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) c += __shfl_xor(c, o);
      if (i == 0 && uv[r] && c != 0) atomicAdd(a.rank + ub0 + 4 * g + r, c);
    }
  }
  if (K > 0) {
    for (int e = lane; e < 16 * K; e += RG_WAVE) {
      const long long b = ub0 + e / K;
      if (b < a.B) part[((long long)slice * a.B + b) * K + e % K] = list[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// merge of the slices' lists, per user
// ------------------------------------------------------------------------------------------------
template <bool LIST>
__global__ __launch_bounds__(TK_MERGE_THREADS) void tk_merge_kernel(const tk_key* __restrict__ part, int slices, int B, int K, int n2,
                                                                    long long first_row, const int64_t* __restrict__ rows,
                                                                    int64_t* __restrict__ ids, float* __restrict__ scores) {
  extern __shared__ __align__(16) unsigned char tk_lds[];
  tk_key* keys = reinterpret_cast<tk_key*>(tk_lds);
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int e = tid; e < n2; e += TK_MERGE_THREADS)
    keys[e] = e < slices * K ? part[((long long)(e / K) * B + b) * K + e % K] : 0;
  __syncthreads();
  // bitonic sort, descending
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < n2; e += TK_MERGE_THREADS) {
        const int p = e ^ j;
        if (p > e) {
          const tk_key x = keys[e], y = keys[p];
          if (((e & k) == 0) ? x < y : x > y) { keys[e] = y; keys[p] = x; }
        }
      }
      __syncthreads();
    }
  for (int e = tid; e < K; e += TK_MERGE_THREADS) {
    const tk_key k = keys[e];
    if (LIST) {
      if (ids) ids[(long long)b * K + e] = k ? (long long)rows[tk_key_row(k)] : -1;          // position in the list -> table row
    } else if (ids) ids[(long long)b * K + e] = k ? first_row + (long long)tk_key_row(k) : -1;
    if (scores) scores[(long long)b * K + e] = k ? tk_key_score(k) : -INFINITY;
  }
}

size_t tk_tscore_bytes(int B) { return ((size_t)B * sizeof(float) + 255) & ~(size_t)255; }
bool tk_shape_ok(int B, int d, long long n_rows, int K) {
  return B >= 1 && (d == 64 || d == 128 || d == 256) && K >= 0 && K <= TK_MAX_K && n_rows >= 1 && n_rows < (1LL << 31);
}

// the first position p of rows that is outside [0, table_rows) or not above rows[p - 1] -> *bad (preset to ~0)
__global__ __launch_bounds__(256) void tk_list_check_kernel(const int64_t* __restrict__ rows, long long n, long long table_rows,
                                                            unsigned long long* __restrict__ bad) {
  const long long step = (long long)gridDim.x * blockDim.x;
  tk_list_check(rows, n, table_rows, bad, (long long)blockIdx.x * blockDim.x + threadIdx.x, step);
}

constexpr size_t TK_LIST_WORD_BYTES = 256;          // the check kernel's word, between tscore and the slices' keys

// LIST: a describes the list's positions (first_row = 0, n_rows = n_list), rows the list, table_rows the table
template <typename T, int D, bool LIST>
int tk_launch(const rg_topk_args& a, const int64_t* rows, long long table_rows, hipStream_t s) {
  float* tscore = reinterpret_cast<float*>(a.workspace);
  tk_key* part = reinterpret_cast<tk_key*>(reinterpret_cast<unsigned char*>(a.workspace) + tk_tscore_bytes(a.B) + (LIST ? TK_LIST_WORD_BYTES : 0));
  const int nub = (a.B + TK_UB - 1) / TK_UB;
  if (a.rank) hipLaunchKernelGGL((tk_gather_kernel<T, D, LIST>), dim3(nub), dim3(TK_THREADS), 0, s, a, rows, table_rows, tscore);
  const int slices = tk_slices(a.B);
  const long long ntiles = (a.n_rows + 15) / 16;
  const long long tps = (ntiles + slices - 1) / slices;
  const int used = (int)((ntiles + tps - 1) / tps);            // slices that hold a tile (the others would write empty lists)
  const size_t lds = (size_t)TK_WAVES * 16 * a.K * sizeof(tk_key);
  auto k = tk_main_kernel<T, D, LIST>;
  hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, dim3(nub, used), dim3(TK_THREADS), lds, s, a, rows, tscore, part, tps);
  if (a.K > 0) {
    int n2 = 1;
    while (n2 < used * a.K) n2 <<= 1;
    const size_t mlds = (size_t)n2 * sizeof(tk_key);
    auto m = tk_merge_kernel<LIST>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(m), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlds);
    hipLaunchKernelGGL(m, dim3(a.B), dim3(TK_MERGE_THREADS), mlds, s, part, used, a.B, a.K, n2, a.first_row, rows, a.topk_ids,
                       a.topk_scores);
  }
  RG_CHECK_LAUNCH();
  return 0;
}

template <typename T, bool LIST>
int tk_dispatch(const rg_topk_args& a, const int64_t* rows, long long table_rows, hipStream_t s) {
  switch (a.d) {
    case 64: return tk_launch<T, 64, LIST>(a, rows, table_rows, s);
    case 128: return tk_launch<T, 128, LIST>(a, rows, table_rows, s);
    case 256: return tk_launch<T, 256, LIST>(a, rows, table_rows, s);
  }
  return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_scores: d must be 64, 128 or 256");
}

}  // namespace

extern "C" size_t rg_topk_workspace(int B, int d, long long n_rows, int K) {
  if (!tk_shape_ok(B, d, n_rows, K)) return 0;
  return tk_tscore_bytes(B) + (size_t)tk_slices(B) * (size_t)B * (size_t)K * sizeof(tk_key);
}

extern "C" int rg_topk_scores(const rg_topk_args* a, int dtype, void* stream) {
  static thread_local char msg[200];
  if (!a || !a->h || !a->table) return rg_set_error_msg(RG_ERR_INVALID, "topk_scores: h and table are required");
  if (a->B <= 0) return 0;
  if (dtype != RG_BF16 && dtype != RG_X3) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_scores: dtype must be RG_BF16 or RG_X3");
  if (a->d != 64 && a->d != 128 && a->d != 256) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_scores: d must be 64, 128 or 256");
  if (a->K < 0 || a->K > TK_MAX_K) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_scores: K must be in [0, 128]");
  if (a->n_rows < 1 || a->n_rows >= (1LL << 31) || a->first_row < 0)
    return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_scores: n_rows must be in [1, 2^31) and first_row >= 0");
  if (a->K > 0 && !a->topk_ids && !a->topk_scores) return rg_set_error_msg(RG_ERR_INVALID, "topk_scores: K > 0 needs topk_ids or topk_scores");
  if (a->K == 0 && !a->rank) return rg_set_error_msg(RG_ERR_INVALID, "topk_scores: K == 0 needs rank");
  if (a->rank && !a->target) return rg_set_error_msg(RG_ERR_INVALID, "topk_scores: rank needs target");
  if ((a->excl == nullptr) != (a->excl_off == nullptr)) return rg_set_error_msg(RG_ERR_INVALID, "topk_scores: excl and excl_off come together");
  const size_t need = rg_topk_workspace(a->B, a->d, a->n_rows, a->K);
  if (!a->workspace || a->workspace_bytes < need) {
    snprintf(msg, sizeof(msg), "topk_scores: workspace of %zu bytes needed, %zu given", need, a->workspace_bytes);
    return rg_set_error_msg(RG_ERR_INVALID, msg);
  }
  hipStream_t s = (hipStream_t)stream;
  if (a->rank) {
    // the targets index the table: checked on the host before anything is launched (one small copy and a wait on the stream)
    std::vector<long long> tg((size_t)a->B);
    hipError_t e = hipMemcpyAsync(tg.data(), a->target, sizeof(long long) * (size_t)a->B, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return rg_set_error(e, __func__);
    for (int b = 0; b < a->B; ++b)
      if (tg[b] < a->first_row || tg[b] >= a->first_row + a->n_rows) {
        snprintf(msg, sizeof(msg), "topk_scores: target[%d] = %lld is outside the catalogue rows [%lld, %lld)", b, tg[b], a->first_row,
                 a->first_row + a->n_rows);
        return rg_set_error_msg(RG_ERR_UNSUPPORTED, msg);
      }
  }
  if (dtype == RG_BF16) return tk_dispatch<__bf16, false>(*a, nullptr, 0, s);
  return tk_dispatch<x3, false>(*a, nullptr, 0, s);
}

// the candidate-list entry points (tests/test_topk_cpu.py pins the one-line extern "C" definitions of this file to the two above)
extern "C" {

size_t rg_topk_list_workspace(int B, int d, long long n_list, int K) {
  if (!tk_shape_ok(B, d, n_list, K)) return 0;
  return tk_tscore_bytes(B) + TK_LIST_WORD_BYTES + (size_t)tk_slices(B) * (size_t)B * (size_t)K * sizeof(tk_key);
}

int rg_topk_list(const rg_topk_list_args* a, int dtype, void* stream) {
  static thread_local char msg[200];
  if (!a || !a->h || !a->table) return rg_set_error_msg(RG_ERR_INVALID, "topk_list: h and table are required");
  if (a->B <= 0) return 0;
  if (dtype != RG_BF16 && dtype != RG_X3) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_list: dtype must be RG_BF16 or RG_X3");
  if (a->d != 64 && a->d != 128 && a->d != 256) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_list: d must be 64, 128 or 256");
  if (a->K < 0 || a->K > TK_MAX_K) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_list: K must be in [0, 128]");
  if (a->n_list < 1 || a->n_list >= (1LL << 31)) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_list: n_list must be in [1, 2^31)");
  if (a->table_rows < 1 || a->table_rows >= (1LL << 31)) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_list: table_rows must be in [1, 2^31)");
  if (!a->rows) return rg_set_error_msg(RG_ERR_INVALID, "topk_list: rows is required");
  if (a->K > 0 && !a->topk_ids && !a->topk_scores) return rg_set_error_msg(RG_ERR_INVALID, "topk_list: K > 0 needs topk_ids or topk_scores");
  if (a->K == 0 && !a->rank) return rg_set_error_msg(RG_ERR_INVALID, "topk_list: K == 0 needs rank");
  if (a->rank && !a->target) return rg_set_error_msg(RG_ERR_INVALID, "topk_list: rank needs target");
  if ((a->excl == nullptr) != (a->excl_off == nullptr)) return rg_set_error_msg(RG_ERR_INVALID, "topk_list: excl and excl_off come together");
  const size_t need = rg_topk_list_workspace(a->B, a->d, a->n_list, a->K);
  if (!a->workspace || a->workspace_bytes < need) {
    snprintf(msg, sizeof(msg), "topk_list: workspace of %zu bytes needed, %zu given", need, a->workspace_bytes);
    return rg_set_error_msg(RG_ERR_INVALID, msg);
  }
  hipStream_t s = (hipStream_t)stream;
  // the list is checked where it lives: one small kernel, its word (and the targets, when ranks are wanted) copied back, one wait
  unsigned long long* bad_d = reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(a->workspace) + tk_tscore_bytes(a->B));
  unsigned long long bad = 0;
  std::vector<long long> tg(a->rank ? (size_t)a->B : 0);
  hipError_t e = hipMemsetAsync(bad_d, 0xFF, sizeof(bad), s);
  if (e != hipSuccess) return rg_set_error(e, __func__);
  const long long blocks = (a->n_list + 255) / 256;
  hipLaunchKernelGGL(tk_list_check_kernel, dim3((unsigned int)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, a->rows, a->n_list,
                     a->table_rows, bad_d);
  RG_CHECK_LAUNCH();
  e = hipMemcpyAsync(&bad, bad_d, sizeof(bad), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && a->rank) e = hipMemcpyAsync(tg.data(), a->target, sizeof(long long) * (size_t)a->B, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return rg_set_error(e, __func__);
  if (bad != ~0ull) {
    // the refusal's message wants the offending value and its predecessor: two more words, on this path only
    const long long p = (long long)bad;
    long long v[2] = {0, 0};
    e = hipMemcpyAsync(v, a->rows + (p > 0 ? p - 1 : 0), sizeof(long long) * (p > 0 ? 2 : 1), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return rg_set_error(e, __func__);
    const long long cur = p > 0 ? v[1] : v[0];
    if (cur < 0 || cur >= a->table_rows)
      snprintf(msg, sizeof(msg), "topk_list: rows[%lld] = %lld is outside the table rows [0, %lld)", p, cur, a->table_rows);
    else
      snprintf(msg, sizeof(msg), "topk_list: rows must be strictly ascending (rows[%lld] = %lld after %lld)", p, cur, v[0]);
    return rg_set_error_msg(RG_ERR_INVALID, msg);
  }
  for (size_t b = 0; b < tg.size(); ++b)
    if (tg[b] < 0 || tg[b] >= a->table_rows) {
      snprintf(msg, sizeof(msg), "topk_list: target[%zu] = %lld is outside the table rows [0, %lld)", b, tg[b], a->table_rows);
      return rg_set_error_msg(RG_ERR_UNSUPPORTED, msg);
    }
  rg_topk_args r = {};
  r.h = a->h; r.table = a->table;
  r.first_row = 0; r.n_rows = a->n_list;          // the kernels' catalogue: the positions of the list
  r.target = a->target; r.excl = a->excl; r.excl_off = a->excl_off;
  r.topk_ids = a->topk_ids; r.topk_scores = a->topk_scores; r.rank = a->rank;
  r.workspace = a->workspace; r.workspace_bytes = a->workspace_bytes;
  r.B = a->B; r.d = a->d; r.K = a->K;
  if (dtype == RG_BF16) return tk_dispatch<__bf16, true>(r, a->rows, a->table_rows, s);
  return tk_dispatch<x3, true>(r, a->rows, a->table_rows, s);
}

}  // extern "C"

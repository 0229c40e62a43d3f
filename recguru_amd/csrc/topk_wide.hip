// Wide top-K: per user the K <= 1024 best catalogue rows of h @ table.T, never forming [B, n_rows] (include/recguru_hip.h,
// rg_topk_wide).  csrc/topk.hip keeps K keys per (slice, user) in LDS and rescans them for every insertion: its cost and its LDS
// grow with K and stop at 128.  Here the K-th largest key is FOUND, not maintained: a most-significant-digit-first radix select on the
// 64-bit key of topk_common.hip.h, the scores recomputed in every pass (a pass is the catalogue walk of tk_main_kernel: same
// tk_scores(), same prefetch, same slices), then one pass that collects the keys at or above the bound and a sort per user.
//
//   per-user state (workspace): prefix = the decided high bits of the K-th key (8 per level), above = eligible keys strictly above
//       the prefix bucket, done, cursor (collect), levels (passes that did work for this user).
//   tkw_level_kernel    grid (user blocks of 64, slices), a wave owns 16 users.  Every key that matches its user's prefix adds 1 to
//       the user's 256-bin histogram of the next 8 key bits (LDS, per wave: 16 KB), flushed with integer atomicAdd to hist [B, 256].
//       A wave whose 16 users are all done returns before it loads anything.
//   tkw_excl_kernel     (exclusion CSR given) one wave per 16 users, as tk_gather_kernel: each user's excluded ids inside the
//       catalogue / list are scored through tk_scores() (column i of a tile whose diagonal is read -- the bits of the walk), and a key
//       that matches the prefix takes 1 off its bin.  The walk never searches an exclusion run.
//   tkw_choose_kernel   one wave per user: scans the bins from the top, extends the prefix by the digit whose bucket holds the
//       (K - above)-th key, clears the bins.  done when above + bucket <= TKW_CAP; fewer than K eligible keys: bound 0, done.
//       Keys are distinct, so after 7 levels (56 bits) a bucket holds <= 256 keys and above < K <= 1024: every user is done --
//       the host enqueues 7 levels, and the number that do work is decided on the device (typical data: 2 - 4).
//   tkw_collect_kernel  the walk once more: a key >= the user's bound is looked up in the exclusion run (only then) and appended to
//       the user's [TKW_CAP] buffer through an integer cursor.  By construction the count fits; the index is checked before the
//       store anyway -- a key that would not fit is dropped and bit 0 of the fault word (workspace offset 0) is set.
//   tkw_sort_kernel     one workgroup per user: bitonic sort in LDS, the first K decoded (through rows in the list form).
//
// Integer atomics only: counts and the SET of collected keys do not depend on the order of arrival, the sort orders distinct keys.
// The unit does not include the deterministic-reduction header; the same object serves both libraries.  A kernel reads only what
// earlier launches on the stream wrote; every loop is bounded by the shape.
//
// Workspace: 256 + align256(32 B) + B (1024 + 16384) bytes: head (fault word at 0, list-check word at 128), state, bins, buffers.
#include "rg_common.hip.h"
#include "topk_common.hip.h"
#include "../../include/recguru_hip.h"

namespace {

constexpr int TKW_MAX_K = 1024;
constexpr int TKW_CAP = 2048;               // collect buffer per user, keys
constexpr int TKW_BINS = 256;               // 8 key bits per level
constexpr int TKW_LEVELS = 7;
constexpr int TKW_SORT_THREADS = 256;
constexpr size_t TKW_HEAD_BYTES = 256;
constexpr size_t TKW_LIST_WORD_AT = 128;

constexpr unsigned int TKW_FAULT_OVERFLOW = 1u, TKW_FAULT_BINS = 2u, TKW_FAULT_NOT_DONE = 4u;

struct tkw_state {
  tk_key prefix;                 // decided bits, the rest 0: the lower bound of the collect pass once done
  int above;                     // eligible keys strictly above the prefix bucket (< K)
  int done;
  unsigned int cursor;           // keys the collect pass offered
  int levels;                    // levels that did work for this user
  int pad[2];
};
static_assert(sizeof(tkw_state) == 32, "the header states 32 bytes of state per user");

struct tkw_args {
  const void* h;
  const void* table;
  long long first_row, n_rows;   // list form: 0, n_list (the catalogue is the positions of the list)
  const int64_t* rows;
  const int64_t* excl;
  const int64_t* excl_off;
  tkw_state* st;
  unsigned int* hist;            // [B, TKW_BINS]
  tk_key* buf;                   // [B, TKW_CAP]
  unsigned int* fault;
  int B, K;
};

// position of id in the ascending list rows[0, n), -1 if it is not a member
__device__ __forceinline__ long long tkw_list_pos(const int64_t* __restrict__ rows, long long n, long long id) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (rows[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && rows[lo] == id) ? lo : -1;
}

// does any of the wave's 16 users still select?  (lane i looks at user ub0 + i)
__device__ __forceinline__ bool tkw_wave_live(const tkw_state* __restrict__ st, long long ub0, int B, int i) {
  const long long b = ub0 + i;
  return __ballot(b < B && st[b].done == 0) != 0;
}

// ------------------------------------------------------------------------------------------------
// one level: the histogram of the next 8 key bits over the keys that match the prefix
// ------------------------------------------------------------------------------------------------
template <typename T, int D, bool LIST>
__global__ __launch_bounds__(TK_THREADS) void tkw_level_kernel(tkw_args a, int level, long long tiles_per_slice) {
  extern __shared__ __align__(16) unsigned char tkw_lds[];
  constexpr int KS = D / 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const long long ub0 = ((long long)blockIdx.x * TK_WAVES + wave) * 16;
  if (ub0 >= a.B) return;                                      // (no workgroup barrier below: the waves are independent)
  if (!tkw_wave_live(a.st, ub0, a.B, i)) return;
  const int slice = blockIdx.y;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.table) + a.first_row * D;
  unsigned int* bins = reinterpret_cast<unsigned int*>(tkw_lds) + (size_t)wave * 16 * TKW_BINS;        // [16][TKW_BINS]
  for (int e = lane; e < 16 * TKW_BINS; e += RG_WAVE) bins[e] = 0;
  __builtin_amdgcn_wave_barrier();

  typename OpT<T>::type ha[KS];
  tk_load_users<T, D>(ha, H, ub0 + i, a.B, g);
  // the lane's four users 4 g + r
  bool act[4];
  tk_key pre[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long b = ub0 + 4 * g + r;
    act[r] = b < a.B && a.st[b].done == 0;
    pre[r] = act[r] ? a.st[b].prefix : 0;
  }
  const int sh = 56 - 8 * level;                                // the level's digit: key bits [sh, sh + 8)
  const tk_key himask = level ? (~0ull << (sh + 8)) : 0ull;      // the decided bits

  const long long ntiles = (a.n_rows + 15) / 16;
  const long long tile0 = (long long)slice * tiles_per_slice;
  const long long tile1 = tile0 + tiles_per_slice < ntiles ? tile0 + tiles_per_slice : ntiles;
  Frag<T> cur[KS], nxt[KS];
  int id_nxt = -1;                                             // LIST: as in tk_main_kernel, the id load runs two tiles ahead
  const unsigned int n_list = (unsigned int)a.n_rows;
  if (tile0 < tile1) {
    const long long row = tile0 * 16 + i;
    if (LIST) {
      tk_load_row<T, D>(cur, W, tk_list_id(a.rows, (unsigned int)row, n_list), g);
      if (tile0 + 1 < tile1) id_nxt = tk_list_id(a.rows, (unsigned int)row + 16, n_list);
    } else {
      tk_load_row<T, D>(cur, W, row < a.n_rows ? row : -1, g);
    }
  }
  for (long long tile = tile0; tile < tile1; ++tile) {
    if (tile + 1 < tile1) {
      const long long row = (tile + 1) * 16 + i;
      if (LIST) {
        tk_load_row<T, D>(nxt, W, id_nxt, g);
        if (tile + 2 < tile1) id_nxt = tk_list_id(a.rows, (unsigned int)row + 16, n_list);
      } else {
        tk_load_row<T, D>(nxt, W, row < a.n_rows ? row : -1, g);
      }
    }
    const f32x4 acc = tk_scores<T, KS>(ha, cur);
    const long long row = tile * 16 + i;                       // row in the catalogue (< 2^31); LIST: position in the list
    const bool iv = row < a.n_rows;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const tk_key key = tk_make_key(acc[r], (unsigned int)row);
      if (iv && act[r] && ((key ^ pre[r]) & himask) == 0)
        atomicAdd(&bins[(4 * g + r) * TKW_BINS + (int)((key >> sh) & (TKW_BINS - 1))], 1u);
    }
    if (tile + 1 < tile1) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) cur[ks] = nxt[ks];
    }
  }

  __builtin_amdgcn_wave_barrier();
  for (int e = lane; e < 16 * TKW_BINS; e += RG_WAVE) {
    const unsigned int v = bins[e];
    const long long b = ub0 + e / TKW_BINS;
    if (v != 0 && b < a.B) atomicAdd(a.hist + b * TKW_BINS + e % TKW_BINS, v);
  }
}

// ------------------------------------------------------------------------------------------------
// the excluded ids' share of a level's histogram, taken off
// ------------------------------------------------------------------------------------------------
template <typename T, int D, bool LIST>
__global__ __launch_bounds__(TK_THREADS) void tkw_excl_kernel(tkw_args a, int level) {
  constexpr int KS = D / 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const long long ub0 = ((long long)blockIdx.x * TK_WAVES + wave) * 16;
  if (ub0 >= a.B) return;
  if (!tkw_wave_live(a.st, ub0, a.B, i)) return;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.table);
  typename OpT<T>::type ha[KS];
  tk_load_users<T, D>(ha, H, ub0 + i, a.B, g);

  // column i of every tile belongs to user ub0 + i
  const long long b = ub0 + i;
  const bool live = b < a.B && a.st[b].done == 0;
  const tk_key pre = live ? a.st[b].prefix : 0;
  const int sh = 56 - 8 * level;
  const tk_key himask = level ? (~0ull << (sh + 8)) : 0ull;
  const long long row_end = a.first_row + a.n_rows;
  long long e0 = 0, len = 0;
  if (live) {
    e0 = a.excl_off[b];
    len = a.excl_off[b + 1] - e0;
  }
  long long maxlen = len;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const long long other = __shfl_xor(maxlen, o);
    maxlen = other > maxlen ? other : maxlen;
  }
  for (long long j = 0; j < maxlen; ++j) {
    long long id = -1, pos = -1;                                // pos: row in the catalogue / position in the list (the key's low word)
    if (j < len) {
      id = a.excl[e0 + j];
      if (j > 0 && a.excl[e0 + j - 1] == id) id = -1;           // (the run is sorted: a repeated id counts once)
      if (LIST) pos = id >= 0 ? tkw_list_pos(a.rows, a.n_rows, id) : -1;
      else pos = (id >= a.first_row && id < row_end) ? id - a.first_row : -1;
      if (pos < 0) id = -1;                                     // outside the catalogue / not in the list: no share
    }
    Frag<T> wb[KS];
    tk_load_row<T, D>(wb, W, id, g);
    const f32x4 acc = tk_scores<T, KS>(ha, wb);
    // the diagonal element sits in lane (i >> 2, i), reg i & 3: picked with masks, as in tk_gather_kernel
    unsigned int sb = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) sb |= __float_as_uint(acc[r]) & (0u - (unsigned int)((i & 3) == r));
    const tk_key key = tk_make_key(__uint_as_float(sb), (unsigned int)pos);
    if (id >= 0 && g == (i >> 2) && ((key ^ pre) & himask) == 0)
      atomicSub(a.hist + b * TKW_BINS + (int)((key >> sh) & (TKW_BINS - 1)), 1u);
  }
}

// ------------------------------------------------------------------------------------------------
// the digit whose bucket holds the (K - above)-th key
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tkw_choose_kernel(tkw_state* __restrict__ st, unsigned int* __restrict__ hist,
                                                         unsigned int* __restrict__ fault, int B, int K, int level) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + wave;
  if (b >= B) return;
  if (st[b].done != 0) return;
  const tk_key prefix = st[b].prefix;
  const unsigned int above = (unsigned int)st[b].above;
  const unsigned int need = (unsigned int)K - above;            // >= 1
  // lane l holds bins 4 l .. 4 l + 3; they are cleared for the next level
  uint4* hp = reinterpret_cast<uint4*>(hist + b * TKW_BINS) + lane;
  const uint4 v = *hp;
  *hp = make_uint4(0u, 0u, 0u, 0u);
  const unsigned int c[4] = {v.x, v.y, v.z, v.w};
  const unsigned int mine = c[0] + c[1] + c[2] + c[3];
  unsigned int inc = mine;                                      // keys in the bins of lanes >= lane
#pragma unroll
  for (int o = 1; o < RG_WAVE; o <<= 1) {
    const unsigned int t = __shfl_down(inc, o);
    if (lane + o < RG_WAVE) inc += t;
  }
  unsigned int run = inc - mine;                                // keys in higher bins than the one looked at
  int digit = -1;
  unsigned int dabove = 0, dcount = 0;
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    if (digit < 0 && run < need && need <= run + c[j]) {
      digit = 4 * lane + j;
      dabove = run;
      dcount = c[j];
    }
    run += c[j];
  }
  const bool any = __ballot(digit >= 0) != 0;
  if (digit >= 0) {                                             // one lane at the most: the bins' running sum crosses need once
    const unsigned int na = above + dabove;
    st[b].prefix = prefix | ((tk_key)(unsigned int)digit << (56 - 8 * level));
    st[b].above = (int)na;
    st[b].done = (na + dcount <= (unsigned int)TKW_CAP || level == TKW_LEVELS - 1) ? 1 : 0;
    st[b].levels = level + 1;
  }
  if (!any && lane == 0) {
    // fewer keys than asked for.  Level 0: fewer than K eligible ids, all of them are wanted (bound 0; K <= TKW_CAP).  Deeper, the
    // bucket was counted larger a level ago: the bins disagree with themselves -- the user keeps its bound, the fault word says so
    if (level != 0) atomicOr(fault, TKW_FAULT_BINS);
    st[b].done = 1;
    st[b].levels = level + 1;
  }
}

// ------------------------------------------------------------------------------------------------
// the keys at or above the bound
// ------------------------------------------------------------------------------------------------
template <typename T, int D, bool LIST>
__global__ __launch_bounds__(TK_THREADS) void tkw_collect_kernel(tkw_args a, long long tiles_per_slice) {
  constexpr int KS = D / 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const long long ub0 = ((long long)blockIdx.x * TK_WAVES + wave) * 16;
  if (ub0 >= a.B) return;
  const int slice = blockIdx.y;
  const T* __restrict__ H = reinterpret_cast<const T*>(a.h);
  const T* __restrict__ W = reinterpret_cast<const T*>(a.table) + a.first_row * D;
  typename OpT<T>::type ha[KS];
  tk_load_users<T, D>(ha, H, ub0 + i, a.B, g);
  bool uv[4];
  tk_key lo[4];
  long long e0[4], e1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long b = ub0 + 4 * g + r;
    uv[r] = b < a.B;
    lo[r] = uv[r] ? a.st[b].prefix : ~0ull;
    if (uv[r] && a.st[b].done == 0) {                           // (cannot happen after TKW_LEVELS levels: nothing is collected for it)
      uv[r] = false;
      if (i == 0 && slice == 0) atomicOr(a.fault, TKW_FAULT_NOT_DONE);
    }
    e0[r] = (a.excl && uv[r]) ? a.excl_off[b] : 0;
    e1[r] = (a.excl && uv[r]) ? a.excl_off[b + 1] : 0;
  }

  const long long ntiles = (a.n_rows + 15) / 16;
  const long long tile0 = (long long)slice * tiles_per_slice;
  const long long tile1 = tile0 + tiles_per_slice < ntiles ? tile0 + tiles_per_slice : ntiles;
  Frag<T> cur[KS], nxt[KS];
  int id_nxt = -1;
  const unsigned int n_list = (unsigned int)a.n_rows;
  if (tile0 < tile1) {
    const long long row = tile0 * 16 + i;
    if (LIST) {
      tk_load_row<T, D>(cur, W, tk_list_id(a.rows, (unsigned int)row, n_list), g);
      if (tile0 + 1 < tile1) id_nxt = tk_list_id(a.rows, (unsigned int)row + 16, n_list);
    } else {
      tk_load_row<T, D>(cur, W, row < a.n_rows ? row : -1, g);
    }
  }
  for (long long tile = tile0; tile < tile1; ++tile) {
    if (tile + 1 < tile1) {
      const long long row = (tile + 1) * 16 + i;
      if (LIST) {
        tk_load_row<T, D>(nxt, W, id_nxt, g);
        if (tile + 2 < tile1) id_nxt = tk_list_id(a.rows, (unsigned int)row + 16, n_list);
      } else {
        tk_load_row<T, D>(nxt, W, row < a.n_rows ? row : -1, g);
      }
    }
    const f32x4 acc = tk_scores<T, KS>(ha, cur);
    const long long row = tile * 16 + i;
    const bool iv = row < a.n_rows;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const tk_key key = tk_make_key(acc[r], (unsigned int)row);
      bool pass = iv && uv[r] && key >= lo[r];
      if (pass && a.excl) pass = !tk_excluded(a.excl, e0[r], e1[r], LIST ? (long long)a.rows[(unsigned int)row] : a.first_row + row);
      if (pass) {
        const long long b = ub0 + 4 * g + r;
        const unsigned int at = atomicAdd(&a.st[b].cursor, 1u);
        if (at < (unsigned int)TKW_CAP) a.buf[b * TKW_CAP + at] = key;
        else atomicOr(a.fault, TKW_FAULT_OVERFLOW);
      }
    }
    if (tile + 1 < tile1) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) cur[ks] = nxt[ks];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// sort and decode, per user
// ------------------------------------------------------------------------------------------------
template <bool LIST>
__global__ __launch_bounds__(TKW_SORT_THREADS) void tkw_sort_kernel(const tkw_state* __restrict__ st, const tk_key* __restrict__ buf, int K,
                                                                    long long first_row, const int64_t* __restrict__ rows,
                                                                    int64_t* __restrict__ ids, float* __restrict__ scores) {
  __shared__ tk_key keys[TKW_CAP];
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned int offered = st[b].cursor;
  const int cnt = offered < (unsigned int)TKW_CAP ? (int)offered : TKW_CAP;
  int n2 = 1;
  while (n2 < cnt) n2 <<= 1;                                   // <= TKW_CAP
  for (int e = tid; e < n2; e += TKW_SORT_THREADS) keys[e] = e < cnt ? buf[(long long)b * TKW_CAP + e] : 0;
  __syncthreads();
  // bitonic sort, descending
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < n2; e += TKW_SORT_THREADS) {
        const int p = e ^ j;
        if (p > e) {
          const tk_key x = keys[e], y = keys[p];
          if (((e & k) == 0) ? x < y : x > y) { keys[e] = y; keys[p] = x; }
        }
      }
      __syncthreads();
    }
  for (int e = tid; e < K; e += TKW_SORT_THREADS) {
    const tk_key k = e < n2 ? keys[e] : 0;
    if (LIST) {
      if (ids) ids[(long long)b * K + e] = k ? (long long)rows[tk_key_row(k)] : -1;          // position in the list -> table row
    } else if (ids) ids[(long long)b * K + e] = k ? first_row + (long long)tk_key_row(k) : -1;
    if (scores) scores[(long long)b * K + e] = k ? tk_key_score(k) : -INFINITY;
  }
}

__global__ __launch_bounds__(256) void tkw_list_check_kernel(const int64_t* __restrict__ rows, long long n, long long table_rows,
                                                             unsigned long long* __restrict__ bad) {
  const long long step = (long long)gridDim.x * blockDim.x;
  tk_list_check(rows, n, table_rows, bad, (long long)blockIdx.x * blockDim.x + threadIdx.x, step);
}

size_t tkw_state_bytes(int B) { return ((size_t)B * sizeof(tkw_state) + 255) & ~(size_t)255; }
bool tkw_shape_ok(int B, int d, long long n_rows, int K) {
  return B >= 1 && (d == 64 || d == 128 || d == 256) && K >= 1 && K <= TKW_MAX_K && n_rows >= 1 && n_rows < (1LL << 31);
}

template <typename T, int D, bool LIST>
int tkw_launch(const tkw_args& a, unsigned char* ws, hipStream_t s) {
  const size_t clear = TKW_HEAD_BYTES + tkw_state_bytes(a.B) + (size_t)a.B * TKW_BINS * sizeof(unsigned int);
  hipError_t e = hipMemsetAsync(ws, 0, clear, s);
  if (e != hipSuccess) return rg_set_error(e, __func__);
  const int nub = (a.B + TK_UB - 1) / TK_UB;
  const int slices = tk_slices(a.B);
  const long long ntiles = (a.n_rows + 15) / 16;
  const long long tps = (ntiles + slices - 1) / slices;
  const int used = (int)((ntiles + tps - 1) / tps);            // slices that hold a tile
  const size_t lds = (size_t)TK_WAVES * 16 * TKW_BINS * sizeof(unsigned int);
  auto lv = tkw_level_kernel<T, D, LIST>;
  hipFuncSetAttribute(reinterpret_cast<const void*>(lv), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  for (int level = 0; level < TKW_LEVELS; ++level) {
    hipLaunchKernelGGL(lv, dim3(nub, used), dim3(TK_THREADS), lds, s, a, level, tps);
    if (a.excl) hipLaunchKernelGGL((tkw_excl_kernel<T, D, LIST>), dim3(nub), dim3(TK_THREADS), 0, s, a, level);
    hipLaunchKernelGGL(tkw_choose_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a.st, a.hist, a.fault, a.B, a.K, level);
  }
  hipLaunchKernelGGL((tkw_collect_kernel<T, D, LIST>), dim3(nub, used), dim3(TK_THREADS), 0, s, a, tps);
  return 0;
}

template <typename T, bool LIST>
int tkw_dispatch(const tkw_args& a, int d, unsigned char* ws, int64_t* ids, float* scores, hipStream_t s) {
  int rc = 0;
  switch (d) {
    case 64: rc = tkw_launch<T, 64, LIST>(a, ws, s); break;
    case 128: rc = tkw_launch<T, 128, LIST>(a, ws, s); break;
    case 256: rc = tkw_launch<T, 256, LIST>(a, ws, s); break;
    default: return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_wide: d must be 64, 128 or 256");
  }
  if (rc != 0) return rc;
  hipLaunchKernelGGL(tkw_sort_kernel<LIST>, dim3(a.B), dim3(TKW_SORT_THREADS), 0, s, a.st, a.buf, a.K, a.first_row, a.rows, ids, scores);
  RG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t rg_topk_wide_workspace(int B, int d, long long n_rows, int K) {
  if (!tkw_shape_ok(B, d, n_rows, K)) return 0;
  return TKW_HEAD_BYTES + tkw_state_bytes(B) + (size_t)B * ((size_t)TKW_BINS * sizeof(unsigned int) + (size_t)TKW_CAP * sizeof(tk_key));
}

extern "C" int rg_topk_wide(const rg_topk_wide_args* a, int dtype, void* stream) {
  static thread_local char msg[200];
  if (!a || !a->h || !a->table) return rg_set_error_msg(RG_ERR_INVALID, "topk_wide: h and table are required");
  if (a->B <= 0) return 0;
  const bool list = a->rows != nullptr;
  if (dtype != RG_BF16 && dtype != RG_X3) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_wide: dtype must be RG_BF16 or RG_X3");
  if (a->d != 64 && a->d != 128 && a->d != 256) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_wide: d must be 64, 128 or 256");
  if (a->K < 1 || a->K > TKW_MAX_K) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_wide: K must be in [1, 1024]");
  if (list) {
    if (a->n_list < 1 || a->n_list >= (1LL << 31)) return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_wide: n_list must be in [1, 2^31)");
    if (a->table_rows < 1 || a->table_rows >= (1LL << 31))
      return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_wide: table_rows must be in [1, 2^31)");
  } else if (a->n_rows < 1 || a->n_rows >= (1LL << 31) || a->first_row < 0) {
    return rg_set_error_msg(RG_ERR_UNSUPPORTED, "topk_wide: n_rows must be in [1, 2^31) and first_row >= 0");
  }
  if (!a->topk_ids && !a->topk_scores) return rg_set_error_msg(RG_ERR_INVALID, "topk_wide: topk_ids or topk_scores is required");
  if ((a->excl == nullptr) != (a->excl_off == nullptr)) return rg_set_error_msg(RG_ERR_INVALID, "topk_wide: excl and excl_off come together");
  const long long n = list ? a->n_list : a->n_rows;
  const size_t need = rg_topk_wide_workspace(a->B, a->d, n, a->K);
  if (!a->workspace || a->workspace_bytes < need) {
    snprintf(msg, sizeof(msg), "topk_wide: workspace of %zu bytes needed, %zu given", need, a->workspace_bytes);
    return rg_set_error_msg(RG_ERR_INVALID, msg);
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = reinterpret_cast<unsigned char*>(a->workspace);
  if (list) {
    // the list is checked where it lives, as rg_topk_list does: one small kernel, its word copied back, one wait
    unsigned long long* bad_d = reinterpret_cast<unsigned long long*>(ws + TKW_LIST_WORD_AT);
    unsigned long long bad = 0;
    hipError_t e = hipMemsetAsync(bad_d, 0xFF, sizeof(bad), s);
    if (e != hipSuccess) return rg_set_error(e, __func__);
    const long long blocks = (a->n_list + 255) / 256;
    hipLaunchKernelGGL(tkw_list_check_kernel, dim3((unsigned int)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, a->rows, a->n_list,
                       a->table_rows, bad_d);
    RG_CHECK_LAUNCH();
    e = hipMemcpyAsync(&bad, bad_d, sizeof(bad), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return rg_set_error(e, __func__);
    if (bad != ~0ull) {
      const long long p = (long long)bad;
      long long v[2] = {0, 0};
      e = hipMemcpyAsync(v, a->rows + (p > 0 ? p - 1 : 0), sizeof(long long) * (p > 0 ? 2 : 1), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) return rg_set_error(e, __func__);
      const long long cur = p > 0 ? v[1] : v[0];
      if (cur < 0 || cur >= a->table_rows)
        snprintf(msg, sizeof(msg), "topk_wide: rows[%lld] = %lld is outside the table rows [0, %lld)", p, cur, a->table_rows);
      else
        snprintf(msg, sizeof(msg), "topk_wide: rows must be strictly ascending (rows[%lld] = %lld after %lld)", p, cur, v[0]);
      return rg_set_error_msg(RG_ERR_INVALID, msg);
    }
  }
  tkw_args k = {};
  k.h = a->h; k.table = a->table;
  k.first_row = list ? 0 : a->first_row; k.n_rows = n;          // list form: the kernels' catalogue is the positions of the list
  k.rows = a->rows; k.excl = a->excl; k.excl_off = a->excl_off;
  k.fault = reinterpret_cast<unsigned int*>(ws);
  k.st = reinterpret_cast<tkw_state*>(ws + TKW_HEAD_BYTES);
  k.hist = reinterpret_cast<unsigned int*>(ws + TKW_HEAD_BYTES + tkw_state_bytes(a->B));
  k.buf = reinterpret_cast<tk_key*>(ws + TKW_HEAD_BYTES + tkw_state_bytes(a->B) + (size_t)a->B * TKW_BINS * sizeof(unsigned int));
  k.B = a->B; k.K = a->K;
  if (list) {
    if (dtype == RG_BF16) return tkw_dispatch<__bf16, true>(k, a->d, ws, a->topk_ids, a->topk_scores, s);
    return tkw_dispatch<x3, true>(k, a->d, ws, a->topk_ids, a->topk_scores, s);
  }
  if (dtype == RG_BF16) return tkw_dispatch<__bf16, false>(k, a->d, ws, a->topk_ids, a->topk_scores, s);
  return tkw_dispatch<x3, false>(k, a->d, ws, a->topk_ids, a->topk_scores, s);
}

// knn_common.h — what the three k-NN translation units share: knn_flat.hip
// (the screened flat search), knn_exact.hip (the fp64 paths: small corpus,
// tiled fallback, block-per-query scan, shard merge) and ivf_search.hip.
// Helpers, constants and the fallback bookkeeping live here once; a kernel is
// defined in exactly one unit and reached from the others through the host
// launchers declared at the end.  No kernels in this header.
#pragma once

#include <float.h>
#include <math.h>
#include <stdlib.h>

#include "nrk_common.h"

namespace nrk {

// ------------------------------------------------------------- constants --
constexpr int SMALL_NB = 4096;          // corpus up to here: exact fp64 tile GEMM (small_launch)
constexpr int64_t EXACT_BELOW = 16384;  // nb in (SMALL_NB, EXACT_BELOW): block-per-query fp64 scan
constexpr int FB_TR = 64;               // tiled fallback: rows per staged tile
constexpr int FB_SLOTS_MAX = 16384;     // collect slots per round / tiled-fallback slots per search

// Test hooks (tests/test_knn_gpu.py, tests/test_ivf_gpu.py) that drive the
// rare exact paths on ordinary data; nothing else reads the environment.
//   NRK_FORCE_FALLBACK=1  certify nothing (flat: the collect pass answers)
//   NRK_FORCE_FALLBACK=2  certify nothing and overflow every collect buffer
//                         (the tiled fp64 fallback answers)
//   NRK_FB_CAP=n          tiled-fallback candidates per slot (tiny: the
//                         block-per-query exact kernel answers)
//   NRK_SCREEN16=0        the 32x32x16 kernels for the flat inner-product main
//                         pass and the IVF collect (test_knn_gpu.py
//                         ::test_screen_main_pass_forms, test_ivf_gpu.py
//                         ::test_ivf_collect_forms)
//   NRK_SCREEN_WAVES=4|8  the flat inner-product main pass at padded dim 128,
//                         k <= 8: 4 forces the 256-query (4-wave) workgroups
//                         where the plan would run 512-query (8-wave) ones, 8
//                         forces those below the plan's query count
//                         (test_knn_screen_w8.py; tools/bench_screen.py A/B)
inline int test_hook(const char* name, int dflt) {
  const char* v = getenv(name);
  return v && *v ? atoi(v) : dflt;
}

inline int padded_dim(int d) {
  if (d <= 32) return 32;
  if (d <= 64) return 64;
  if (d <= 128) return 128;
  if (d <= 256) return 256;
  return (int)align_up((size_t)d, 32);
}

__host__ __device__ inline int pow2ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// Tiled fallback: candidates per slot.  Room for 2k + 64 items at least as
// good as the slot's threshold (ties and near-ties); overflow goes to the
// block-per-query scan.  fallback_select_kernel sorts cap x 16 B in LDS.
inline int fallback_cap(int k) {
  int cap = pow2ceil(2 * k + 64);
  if (cap < 512) cap = 512;
  cap = test_hook("NRK_FB_CAP", cap);
  if (cap < 1) cap = 1;
  if (cap > 8192) cap = 8192;
  return cap;
}

// Workspace carving: regions in call order, each aligned to 256 B.  With a
// null base only the offsets advance (the plan's total).
struct Carver {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t count) {
    const size_t o = off;
    off = align_up(off + count * sizeof(T), 256);
    return base ? reinterpret_cast<T*>(base + o) : nullptr;
  }
};

// ------------------------------------------------------- ordered keys --
// Order-preserving map float -> uint32 (larger float, larger key) and back.
// Every finite float and +-inf has a key >= 1 (NaNs aside), so 0 can mark an
// empty slot.
__device__ __forceinline__ uint32_t ordered_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The R-th largest of a wave's 64 x NK keys (slot j of lane l is entry 64 j +
// l; key 0 = empty slot), or 0 if fewer than R are nonzero: exact selection by
// bisection on the key bits, 32 rounds of NK ballot counts.
template <int NK>
__device__ __forceinline__ uint32_t wave_kth_key(const uint32_t (&key)[NK], int R) {
  uint32_t K = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t c = K | (1u << bit);
    int n = 0;
#pragma unroll
    for (int j = 0; j < NK; ++j) n += __popcll(__ballot(key[j] >= c));
    if (n >= R) K = c;
  }
  return K;
}
// Its compaction: with K = wave_kth_key(key, R), calls take(j, pos) on the
// lane holding each selected entry — every key above K, then ties at K in
// (slot, lane) order until R are taken; pos counts 0, 1, ... in (slot, lane)
// order.  K = 0 selects every nonzero key.  Returns the lane's largest key
// left out (0: none).
template <int NK, class Take>
__device__ __forceinline__ uint32_t wave_take_top(const uint32_t (&key)[NK], uint32_t K, int R, Take&& take) {
  int need = R, base = 0;
#pragma unroll
  for (int j = 0; j < NK; ++j) need -= K ? __popcll(__ballot(key[j] > K)) : 0;
  uint32_t kout = 0;
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const unsigned long long eq = K ? __ballot(key[j] == K) : 0ull;
    const bool sel = key[j] > K || (K && key[j] == K && lanes_below(eq) < need);
    const unsigned long long sm = __ballot(sel);
    if (sel) take(j, base + lanes_below(sm));
    else if (key[j] > kout) kout = key[j];
    base += __popcll(sm);
    const int ne = __popcll(eq);
    need -= ne < need ? ne : need;
  }
  return kout;
}

// ------------------------------------------------------- exact scores --
// fp64 score in the oracle's serial order (bit-identical).  One lane per
// candidate row: scalar loads measured faster than float4 ones here (k = 5
// merge 0.086 vs 0.103 ms); many candidates go through staged_rescore instead.
__device__ __forceinline__ double exact_score(const float* __restrict__ qs, const float* __restrict__ x,
                                              int d, bool l2) {
  double acc = 0.0;
  if (!l2) {
    for (int j = 0; j < d; ++j) acc = fma((double)qs[j], (double)x[j], acc);
  } else {
    for (int j = 0; j < d; ++j) {
      double t = (double)qs[j] - (double)x[j];
      acc = fma(t, t, acc);
    }
  }
  return acc;
}

// Exact goodness of n candidate rows (ids[0, n) -> gout[0, n)) by a 256-thread
// block, d a multiple of 4: lane = candidate row, fp64 in the oracle's serial
// order; the rows are staged through LDS (stg: [256][CW + 4] floats) CW columns
// at a time by coalesced float4 loads (one lane per row reading it 4 B at a
// time left every load instruction touching 256 different rows).  qs: the
// query in LDS.  Every thread of the block calls it.
template <int CW>
__device__ __forceinline__ void staged_rescore(float* stg, const int64_t* ids, int n, const float* __restrict__ xb,
                                               int d, const float* qs, int l2, double* gout) {
  const int tid = threadIdx.x;
  for (int r0 = 0; r0 < n; r0 += 256) {
    const int nr = n - r0 < 256 ? n - r0 : 256;
    double acc = 0.0;
    for (int c0 = 0; c0 < d; c0 += CW) {
      const int cw = d - c0 < CW ? d - c0 : CW;
#pragma unroll
      for (int t = 0; t < CW / 4; ++t) {
        const int e = tid + 256 * t, row = e / (CW / 4), c4 = e % (CW / 4);
        if (row < nr && 4 * c4 < cw)
          *reinterpret_cast<float4*>(stg + row * (CW + 4) + 4 * c4) =
              *reinterpret_cast<const float4*>(xb + ids[r0 + row] * d + c0 + 4 * c4);
      }
      __syncthreads();
      if (tid < nr) {
        const float* xr = stg + tid * (CW + 4);
        for (int j = 0; j < cw; j += 4) {
          const float4 v = *reinterpret_cast<const float4*>(xr + j);
          const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (l2) {
              const double t = (double)qs[c0 + j + u] - (double)xv[u];
              acc = fma(t, t, acc);
            } else {
              acc = fma((double)qs[c0 + j + u], (double)xv[u], acc);
            }
          }
        }
      }
      __syncthreads();
    }
    if (tid < nr) gout[r0 + tid] = l2 ? -acc : acc;
  }
}

// One result slot: the score (IP) or distance (L2) of goodness g, the id plus
// the shard offset; an empty slot gets the sentinels (-FLT_MAX / FLT_MAX, -1).
__device__ __forceinline__ void write_result(float* __restrict__ D, int64_t* __restrict__ I, double* __restrict__ S,
                                             int64_t o, bool valid, double g, int64_t id, bool l2, int64_t id_offset) {
  const double s = valid ? (l2 ? -g : g) : (l2 ? DBL_MAX : -DBL_MAX);
  D[o] = valid ? (float)s : (l2 ? FLT_MAX : -FLT_MAX);
  I[o] = valid ? id + id_offset : -1;
  if (S) S[o] = s;
}

// Collect threshold in screened units.  e_k is the exact goodness of a real
// item ranked k-th among exactly scored real items, so the true k-th best is at
// least e_k; every true top-k item x then has screened(x) >= exact(x) - B_q >=
// e_k - B_q (IP), resp. screened = 2 q^.x^ - |x|^2 >= e_k + |q|^2 - B_q (L2,
// goodness = -|q - x|^2), with the flat certificate's error bound B_q.  Rounded
// down to f32 with slack for the fp64 evaluation of the bound itself.
__device__ __forceinline__ float collect_threshold(double ek, const double* __restrict__ qm,
                                                   const float* __restrict__ stats, int dp, int l2) {
  const double nqh = qm[0], nrq = qm[1], qn2 = qm[2];
  const double Xh = stats[0], Rr = stats[1], NX = stats[2];
  const double gam = (double)dp * 0x1p-22;
  const double bip = gam * nqh * Xh + nqh * Rr + nrq * Xh + nrq * Rr;
  // L2: + dp 2^-23 NX for screens whose accumulators start at -|x|^2 / 2
  // (screen16_collect_kernel): up to dp fp32 roundings of a running value that
  // holds half the row norm, doubled with the score
  const double B = l2 ? 2.0 * bip + 0x1p-21 * (NX + nqh * Xh) + (double)dp * 0x1p-23 * NX : bip;
  double t = (l2 ? qn2 + ek : ek) - B;
  t -= 1e-9 * (fabs(t) + fabs(ek) + qn2 + B);
  float f = (float)t;
  if ((double)f > t) f = nextafterf(f, -INFINITY);
  return f < -FLT_MAX ? -FLT_MAX : f;
}

// ------------------------------------------------ fallback bookkeeping --
// Shared by the merge / collect kernels and the tiled fallback.  An
// uncertified query gets a slot s (list[s] = query) and, for s < tslots, the
// exact k-th (goodness, id) known so far: every item of the true top-k is at
// least that good, so the fallback only has to collect those.
struct FbState {
  int* list;        // [nq] queries, in slot order
  int* count;       // [0] = entries pushed, [1] = overflow count (fallback_select)
  int slots;        // slots with candidate storage (n, the tiled fallback's candidate lists)
  int tslots;       // slots with a stored threshold (>= slots)
  double* thr_g;    // [tslots]
  int64_t* thr_i;   // [tslots]
  int* n;           // [slots] candidates seen (may exceed cap)
  int force;        // testing: certify nothing
  __device__ void push(int qi, double g, int64_t i) const {
    const int s = atomicAdd(count, 1);
    list[s] = qi;
    if (s < tslots) {
      thr_g[s] = g;
      thr_i[s] = i;
    }
    if (s < slots) n[s] = 0;
  }
};

// IVF restriction for the exact paths: only items of the query's probed lists
// are eligible (faiss IndexIVF semantics); rows are addressed by id.
struct IvfFb {
  const int64_t* pos2id;    // [n] list-major position -> id (nullptr: flat index)
  const int* pos2list;      // [n]
  const int64_t* list_off;  // [nlist + 1]
  const int64_t* probe;     // [nq][nprobe] probed lists (-1: none)
  int nprobe;
  int nlist;
  int64_t nq;               // queries of the search (0: slot queries unchecked)
  int* err;                 // the search's guard word (GuardCode bits), or nullptr
};

// ------------------------------------------------------------ launchers --
// Each takes what its launch takes and returns an NRK_* code.

// knn_flat.hip
int query_prepare_launch(const float* xq, int64_t nq, int64_t nq_pad, int d, int dp, uint16_t* qh, double* qmeta,
                         int* zero4, int* zero2, hipStream_t st);
// tau_select_kernel for nvals (<= 1024) values per query: grid nq / 4, 256 threads
typedef void (*tau_select_fn_t)(const float* premax, int nvals, int R, int64_t nq, float* tau, const int* ids_in,
                                int* ids_out);
tau_select_fn_t tau_select_fn(int nvals);
// one block per slot; qlist / qcount: the flat collect pass's slot -> query map
int collect_rescore_launch(int nslots, const int* cand_cnt, const int* cand_pos, int cap, const int64_t* pos2id,
                           const float* xq, const float* xb, int d, int k, int l2, const double* lb_g,
                           const int64_t* lb_i, float* D, int64_t* I, double* S, int64_t id_offset, FbState fb,
                           int64_t nq, int64_t n, int* err, const int* qlist, const int* qcount, hipStream_t st);

// knn_exact.hip
struct SmallPlan {  // nb <= SMALL_NB: queries per chunk of the goodness matrix G[chunk][ld]
  int P;            // pow2ceil(nb): small_select_kernel's sort size
  int64_t ld, chunk;
  size_t ws_bytes;
};
SmallPlan make_small_plan(int64_t nq, int64_t nb, int k);
int small_launch(const SmallPlan& p, const float* xq, int64_t nq, const float* xb, int64_t nb, int d, int k, int l2,
                 float* D, int64_t* I, double* S, int64_t id_offset, void* ws, hipStream_t st, int32_t* nfb);
// block-per-query fp64 scan over all nq queries, or over qlist[0, *qcount);
// cnt_out (with cnt_a, cnt_b): publishes the search's two fallback counts
int exact_launch(const float* xq, int64_t nq, const float* xb, int64_t nb, int d, int k, int l2, const int* qlist,
                 const int* qcount, int64_t max_work, float* D, int64_t* I, double* S, int64_t id_offset,
                 hipStream_t st, IvfFb iv = IvfFb{}, int* cnt_out = nullptr, const int* cnt_a = nullptr,
                 const int* cnt_b = nullptr);
// The end of both searches: the tiled fp64 scan for the slots of fb (candidates
// in cand_g / cand_i, cap per slot), the per-slot select (overflow -> ov_list,
// counted in fb.count[1]) and the block-per-query scan of the overflow list.
int fallback_tail(const float* xq, int64_t nq, const float* xb, int64_t nb, int d, int k, int l2, FbState fb,
                  double* cand_g, int64_t* cand_i, int cap, int* ov_list, float* D, int64_t* I, double* S,
                  int64_t id_offset, IvfFb iv, hipStream_t st, int* cnt_out = nullptr, const int* cnt_a = nullptr,
                  const int* cnt_b = nullptr);

}  // namespace nrk

// ivf_search.hip — faiss IndexIVFFlat.search (BASELINE configs[3]; the
// inverted lists of Retrieval.py:21-23).  The caller supplies the probed lists
// (the coarse quantizer's top-nprobe, a flat search over the centroids).
// List-major batching: every (query, probe) pair is grouped under its list,
// each list's probing queries are gathered into a padded bf16 segment, and the
// screen kernels run (list, query tile, list chunk) work items, so each list
// chunk is streamed once per 32*QT*WAVES queries.
//   phase A: lane maxima (screen MODE 4) over each query's nearest lists, the
//            best R rescored exactly -> e_k, a lower bound on the k-th best,
//            and from it the collect threshold (collect_threshold)
//   phase B: collect (screen MODE 3) every probed item at or above the
//            threshold, rescore all of them exactly (collect_rescore), top-k
//   fallback_tail: fp64 scans, restricted to the probed lists, for queries
//            with too few seeds or an overflowed candidate buffer
// Exact by construction: no certificate.  See DESIGN.md "K-IVF-SCAN".
#include "knn_common.h"
#include "screen16.h"

namespace nrk {

__global__ void ivf_count_kernel(const int64_t* __restrict__ probe, int64_t npairs, int nlist, int* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npairs) return;
  const int64_t l = probe[i];
  if (l >= 0 && l < nlist) atomicAdd(&cnt[l], 1);
}

// Contention-free grouping (nlist <= GROUP_LDS_LISTS): GROUP_BLOCKS blocks
// each count their slice of the (query, probe) pairs per list in LDS and write
// one histogram row; the plan kernel turns the rows into per-block offsets; the
// placing blocks re-read their slice and rank inside the block with LDS
// atomics.  (One global atomic per pair on a few hundred list counters cost
// ~50 us per grouping at 131K pairs.)  The order of a list's queries inside its
// segment is arbitrary: every consumer is order-independent.
constexpr int GROUP_BLOCKS = 64;
constexpr int GROUP_LDS_LISTS = 16384;

__global__ __launch_bounds__(1024) void ivf_hist_kernel(const int64_t* __restrict__ probe, int64_t npairs, int nlist,
                                                        int* __restrict__ H) {
  extern __shared__ int hist[];
  for (int l = threadIdx.x; l < nlist; l += blockDim.x) hist[l] = 0;
  __syncthreads();
  const int64_t per = cdiv(npairs, (int64_t)gridDim.x);
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < npairs ? i0 + per : npairs;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    const int64_t l = probe[i];
    if (l >= 0 && l < nlist) atomicAdd(&hist[l], 1);
  }
  __syncthreads();
  for (int l = threadIdx.x; l < nlist; l += blockDim.x) H[(int64_t)blockIdx.x * nlist + l] = hist[l];
}

__global__ __launch_bounds__(1024) void ivf_place_kernel(const int64_t* __restrict__ probe, int64_t npairs, int nlist,
                                                         const int* __restrict__ seg_off, const int* __restrict__ H,
                                                         int* __restrict__ slot_pair) {
  extern __shared__ int base[];
  for (int l = threadIdx.x; l < nlist; l += blockDim.x) base[l] = seg_off[l] + H[(int64_t)blockIdx.x * nlist + l];
  __syncthreads();
  const int64_t per = cdiv(npairs, (int64_t)gridDim.x);
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < npairs ? i0 + per : npairs;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    const int64_t l = probe[i];
    if (l >= 0 && l < nlist) slot_pair[atomicAdd(&base[l], 1)] = (int)i;
  }
}

// One block: per-list query segments (padded to wq rows) and work-item prefix.
// With H (the histogram rows of ivf_hist_kernel), the per-list counts are
// first summed over the GB rows, which become exclusive per-block offsets.
__global__ __launch_bounds__(1024) void ivf_plan_kernel(int* __restrict__ cnt,
                                                        const int64_t* __restrict__ list_off, int nlist, int wq,
                                                        int ch, int* __restrict__ seg_off, int* __restrict__ work_off,
                                                        int* __restrict__ fill, int* __restrict__ H = nullptr,
                                                        int GB = 0) {
  __shared__ int s_seg[1024], s_work[1024];
  const int t = threadIdx.x;
  const int per = (nlist + 1023) / 1024;
  const int lo = t * per < nlist ? t * per : nlist, hi = lo + per < nlist ? lo + per : nlist;
  if (H) {
    for (int l = lo; l < hi; ++l) {
      int run = 0;
      for (int b0 = 0; b0 < GB; b0 += 16) {  // 16 loads in flight
        int v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = b0 + u < GB ? H[(int64_t)(b0 + u) * nlist + l] : 0;
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (b0 + u < GB) {
            H[(int64_t)(b0 + u) * nlist + l] = run;
            run += v[u];
          }
      }
      cnt[l] = run;  // read back below by this same thread
    }
  }
  int ss = 0, sw = 0;
  for (int l = lo; l < hi; ++l) {
    const int rows = (cnt[l] + wq - 1) / wq * wq;
    const int nchl = (int)cdiv(list_off[l + 1] - list_off[l], (int64_t)ch);
    ss += rows;
    sw += rows / wq * nchl;
  }
  s_seg[t] = ss;
  s_work[t] = sw;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int a = t >= o ? s_seg[t - o] : 0, b = t >= o ? s_work[t - o] : 0;
    __syncthreads();
    s_seg[t] += a;
    s_work[t] += b;
    __syncthreads();
  }
  int es = s_seg[t] - ss, ew = s_work[t] - sw;
  for (int l = lo; l < hi; ++l) {
    const int rows = (cnt[l] + wq - 1) / wq * wq;
    const int nchl = (int)cdiv(list_off[l + 1] - list_off[l], (int64_t)ch);
    seg_off[l] = es;
    work_off[l] = ew;
    fill[l] = 0;
    es += rows;
    ew += rows / wq * nchl;
  }
  if (t == 1023) {
    seg_off[nlist] = s_seg[1023];
    work_off[nlist] = s_work[1023];
  }
}

__global__ void ivf_scatter_kernel(const int64_t* __restrict__ probe, int64_t npairs, int nlist,
                                   const int* __restrict__ seg_off, int* __restrict__ fill,
                                   int* __restrict__ slot_pair) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npairs) return;
  const int64_t l = probe[i];
  if (l < 0 || l >= nlist) return;
  slot_pair[seg_off[l] + atomicAdd(&fill[l], 1)] = (int)i;
}

// gathered query rows: one wave per slot row (padding rows are zeroed), a
// grid-stride loop over the rows the grouping produced (seg_off[nlist]; a grid
// sized for the upper bound launched ~50K blocks of which most exited: 25 us)
constexpr int GATHER_BLOCKS = 2048;
__global__ void ivf_gather_kernel(const uint16_t* __restrict__ qh, int dp, int nprobe,
                                  const int* __restrict__ slot_pair, const int* __restrict__ seg_off, int nlist,
                                  int64_t max_rows, uint16_t* __restrict__ qh_ivf, int64_t npairs,
                                  int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t nrows = seg_off[nlist] < max_rows ? seg_off[nlist] : max_rows;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < nrows; row += nw) {
    int pair = slot_pair[row];
    if (pair >= 0 && !guard_ok(pair < npairs, err, GUARD_GATHER_PAIR)) pair = -1;
    const int64_t q = pair >= 0 ? pair / nprobe : 0;
    for (int j = lane * 4; j < dp; j += 256) {
      uint2 v = make_uint2(0u, 0u);
      if (pair >= 0) v = *reinterpret_cast<const uint2*>(qh + q * dp + j);
      *reinterpret_cast<uint2*>(qh_ivf + row * dp + j) = v;
    }
  }
}

// IVF phase A seed: exact rescoring of the R best lane maxima of the nearest
// list (distinct real items) -> e_k = their k-th best exact (goodness, id),
// a lower bound on the true k-th best s_k.  Every true top-k item x then has
// screened(x) >= exact(x) - B >= e_k - B =: T (screened units, rounded down;
// same error bound B_q as the flat certificate), and (e_k, id) is the
// fallback threshold.  Fewer than k seeds: the query goes to the fallback.
__global__ __launch_bounds__(64) void ivf_seed_kernel(const int* __restrict__ seed_pos, int R, int k,
                                                       const int64_t* __restrict__ pos2id,
                                                       const float* __restrict__ xq, const float* __restrict__ xb,
                                                       int d, int l2, const double* __restrict__ qmeta,
                                                       const float* __restrict__ stats, int dp,
                                                       float* __restrict__ thr, double* __restrict__ lb_g,
                                                       int64_t* __restrict__ lb_i, int* __restrict__ cand_cnt,
                                                       int cap, int64_t n, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int P = pow2ceil(R);
  double* g = reinterpret_cast<double*>(smem);
  int64_t* id = reinterpret_cast<int64_t*>(g + P);
  float* qs = reinterpret_cast<float*>(id + P);
  __shared__ int s_valid;
  if (tid == 0) s_valid = 0;
  // one wave per query (a 256-thread block idled 7/8 of its lanes and paid the
  // sort's barriers across four waves)
  for (int i = tid; i < d; i += blockDim.x) qs[i] = xq[(int64_t)q * d + i];
  __syncthreads();
  for (int i = tid; i < P; i += blockDim.x) {
    const int pos = i < R ? seed_pos[(int64_t)q * R + i] : -1;
    if (pos >= 0 && guard_ok(pos < n, err, GUARD_SEED_POS)) {
      const int64_t item = pos2id[pos];
      const double sc = exact_score(qs, xb + item * d, d, l2 != 0);
      g[i] = l2 ? -sc : sc;
      id[i] = item;
      atomicAdd(&s_valid, 1);
    } else {
      g[i] = -INFINITY;
      id[i] = INT64_MAX;
    }
  }
  __syncthreads();
  block_bitonic_sort(g, id, P);
  if (tid != 0) return;
  if (s_valid < k) {  // too few seeds for a bound: no collection, straight to the fallback
    thr[q] = INFINITY;
    lb_g[q] = -INFINITY;
    lb_i[q] = -1;
    cand_cnt[q] = cap + 1;
    return;
  }
  const double ek = g[k - 1];
  thr[q] = collect_threshold(ek, qmeta + 4 * q, stats, dp, l2);
  lb_g[q] = ek;
  lb_i[q] = id[k - 1];
}

struct IvfPlan {
  int dp, qt, M, waves, wq, nqt;
  int wavesB;               // phase B (collect) waves per workgroup: wq = wavesB x 32 x qt
  int qtA, wqA;             // phase A query tiles per wave / queries per work item
  int nA, chA, cmaxA, R;    // phase A: lane maxima (+positions) over the nA nearest lists, R seeds
  int chB, cmaxB, cap;      // phase B: all probed lists, collect above e_k - B
  int fb_slots, fb_cap;
  int64_t nq_pad, max_rows, ubA, ubB;
  size_t total;             // workspace bytes (ivf_carve)
};

// The first region holds 16 ints: the fallback counters [0, 4), the guard word,
// the collect work tickets [8, 16).  nrk_ivf_search_status reads the guard word
// at this fixed byte of the workspace, so the region must stay first.
constexpr int IVF_GUARD_INT = 4;
constexpr size_t IVF_GUARD_BYTE = IVF_GUARD_INT * sizeof(int);

// The search's workspace, one line per region: type and element count, in
// workspace order, each region aligned to 256 B.
struct IvfWs {
  int* fbc;                        // counters, guard word, tickets (above)
  int *cnt, *fill, *hist;          // grouping: per-list counts, fill cursors, per-block histograms
  int *seg, *work, *sp;            // list segments, work-item prefix, slot -> pair
  uint16_t* qh;                    // bf16 queries, padded
  double* qmeta;
  uint16_t* qi;                    // the probing queries gathered list-major
  int64_t* p0;                     // phase A: the nA nearest lists of each query
  float* pt;                       // phase A lane maxima and their positions
  int* pa;
  float* tau;
  int* seed;                       // phase A: positions of the R seeds
  double* lbg;                     // e_k (goodness, id) and the collect threshold
  int64_t* lbi;
  float* thr;
  int *ccnt, *cpos;                // phase B: candidates per query
  int* fbl;                        // tiled fallback: queries, thresholds, candidates
  double* fbt;
  int64_t* fbi;
  int* fbn;
  double* fcg;
  int64_t* fci;
  int* ovl;                        // queries for the block-per-query scan
};
static size_t ivf_carve(char* base, const IvfPlan& p, int64_t nq, int nlist, IvfWs& w) {
  Carver c{base};
  const size_t n = (size_t)nq, slots = (size_t)p.fb_slots, nl = (size_t)nlist;
  const size_t npa = n * p.nA * p.cmaxA * 2;  // lane streams of phase A
  w.fbc = c.take<int>(16);
  w.cnt = c.take<int>(nl);
  w.fill = c.take<int>(nl);
  w.hist = c.take<int>((size_t)GROUP_BLOCKS * nl);
  w.seg = c.take<int>(nl + 1);
  w.work = c.take<int>(nl + 1);
  w.sp = c.take<int>((size_t)p.max_rows);
  w.qh = c.take<uint16_t>((size_t)p.nq_pad * p.dp);
  w.qmeta = c.take<double>(n * 4);
  w.qi = c.take<uint16_t>((size_t)p.max_rows * p.dp);
  w.p0 = c.take<int64_t>(n * p.nA);
  w.pt = c.take<float>(npa);
  w.pa = c.take<int>(npa);
  w.tau = c.take<float>(n);
  w.seed = c.take<int>(n * p.R);
  w.lbg = c.take<double>(n);
  w.lbi = c.take<int64_t>(n);
  w.thr = c.take<float>(n);
  w.ccnt = c.take<int>(n);
  w.cpos = c.take<int>(n * p.cap);
  w.fbl = c.take<int>(n);
  w.fbt = c.take<double>(slots);
  w.fbi = c.take<int64_t>(slots);
  w.fbn = c.take<int>(slots);
  w.fcg = c.take<double>(slots * p.fb_cap);
  w.fci = c.take<int64_t>(slots * p.fb_cap);
  w.ovl = c.take<int>(n);
  return c.off;
}

static IvfPlan make_ivf_plan(int64_t nq, int nprobe, int nlist, int64_t max_list, int d, int k) {
  IvfPlan p;
  memset(&p, 0, sizeof(p));
  p.dp = padded_dim(d);
  p.waves = 4;
  p.M = 1;  // neither phase keeps lane lists (mode 4: lane maxima, mode 3: collect)
  // phase B: two query tiles per wave at k <= 8 (one at DP = 256 or k > 8), 4 waves
  // (256 probing queries per work item at configs[3]).  8 waves (512 per item) cut
  // the configs[3] fetch 6.0 -> 4.0 GB per launch but padded the list segments more
  // (3.66 -> 4.11 padded TF) and ran 3.36 -> 3.79 ms (profiles/r03_ivf_collect_ab.log):
  // the screen is MFMA-bound, not HBM-bound
  p.qt = (k <= 8 && p.dp != 256) ? 2 : 1;
  p.wavesB = 4;
  p.wq = p.wavesB * 32 * p.qt;
  // phase A (lane maxima over the nA nearest lists) runs one query tile per
  // wave: half the work-item padding of the grouped queries and a lighter
  // epilogue.  Phase B keeps p.qt (two tiles share each A fragment).
  p.qtA = 1;
  p.wqA = p.waves * 32 * p.qtA;
  p.nqt = (int)cdiv(nq, p.wq);
  p.nq_pad = (int64_t)p.nqt * p.wq;
  const int64_t ml = max_list > 0 ? max_list : 1;
  const int64_t ch_gib = ((int64_t)1 << 30) / (p.dp * 2) / 64 * 64;  // buffer descriptor range
  // phase A: the nA nearest lists per query in chunks of max_list / 128 items (2 lane
  // streams per chunk and query; more streams -> tighter seeds); tau_select
  // takes <= 1024 values per query
  // (one list per query left too few seeds for some queries: fp64 scans, 3.4 -> 248 ms
  // per search; profiles/r06_ivf_phaseA_ab.log)
  p.nA = nprobe < 2 ? nprobe : 2;
  // chunks scale with the lists (max_list / 128, in [64, 4096] rows): a
  // corpus shard's short lists (the 8-GPU configs[3]: ~4K rows) otherwise
  // gave ~20 lane maxima per query, weak seeds, a low collect threshold and
  // ~3 % of the queries overflowing into the fp64 scan
  // (capped at 4096 rows: at configs[3] (max list 213K) 1024-row chunks made ~5-tile
  // items whose prologues dominated phase A; 0.49 -> 0.41 ms, the exact rescore +0.01
  // ms; ml / 32 starved the seeds: profiles/r04_ivf_phaseA_chunks_ab.log)
  int64_t chA = (int64_t)align_up((size_t)(ml / 128 > 64 ? ml / 128 : 64), 64);
  if (chA > 4096) chA = 4096;
  const int64_t cmax_a = 512 / p.nA;
  if (cdiv(ml, chA) > cmax_a) chA = (int64_t)align_up((size_t)cdiv(ml, cmax_a), 64);
  if (chA > ch_gib) chA = ch_gib;
  p.chA = (int)chA;
  p.cmaxA = (int)cdiv(ml, chA);
  p.R = 2 * k > 32 ? 2 * k : 32;  // seeds rescored exactly
  if (p.R > 2 * p.nA * p.cmaxA) p.R = 2 * p.nA * p.cmaxA;
  if (p.R < 1) p.R = 1;
  // phase B: chunk size only sets the work-item granularity
  int64_t chB = 4096;
  if (chB > ch_gib) chB = ch_gib;
  p.chB = (int)chB;
  p.cmaxB = (int)cdiv(ml, chB);
  p.cap = k > 2048 ? k : 2048;
  const int64_t npairs = nq * nprobe;
  p.max_rows = npairs + (int64_t)nlist * (p.wq - 1);
  p.max_rows = (p.max_rows + p.wq - 1) / p.wq * p.wq;
  // persistent grids over the device work tables (upper bound on the items)
  const int64_t gcap = 2048;
  p.ubA = (cdiv(nq * p.nA, (int64_t)p.wqA) + nlist) * p.cmaxA;
  p.ubB = (cdiv(npairs, (int64_t)p.wq) + nlist) * p.cmaxB;
  if (p.ubA > gcap) p.ubA = gcap;
  if (p.ubB > gcap) p.ubB = gcap;
  p.fb_slots = (int)(nq < FB_SLOTS_MAX ? nq : FB_SLOTS_MAX);  // as the flat plan
  p.fb_cap = fallback_cap(k);
  IvfWs w;
  p.total = ivf_carve(nullptr, p, nq, nlist, w);
  return p;
}

// The search's start-of-call state in ONE launch instead of five blits (each a
// ~4.5 us fill kernel on the stream): the counters and guard word (fbc[0..16)),
// n_fallback, the phase-A probe copy p0 (the nA nearest lists of each query),
// the phase-A lane maxima (all bits set: NaN, never selected), the candidate
// counts and phase A's slot -> pair table (all -1).
__global__ __launch_bounds__(256) void ivf_init_kernel(int* __restrict__ fbc, int32_t* __restrict__ nfb,
                                                       int64_t* __restrict__ p0, const int64_t* __restrict__ probe,
                                                       int64_t nq, int64_t nq_p0, int nprobe, int nA,
                                                       uint32_t* __restrict__ pt, int64_t npt, int* __restrict__ ccnt,
                                                       int* __restrict__ sp, int64_t nsp) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  if (t0 < 16) fbc[t0] = 0;
  if (nfb && t0 < 2) nfb[t0] = 0;
  for (int64_t i = t0; i < nq_p0 * nA; i += stride) p0[i] = probe[(i / nA) * nprobe + i % nA];
  for (int64_t i = t0; i < npt; i += stride) pt[i] = 0xffffffffu;
  for (int64_t i = t0; i < nq; i += stride) ccnt[i] = 0;
  for (int64_t i = t0; i < nsp; i += stride) sp[i] = -1;
}

// group (query, probe) pairs by list and gather the probing queries list-major
// (fill_sp: set the slot -> pair table to -1 first; the first grouping's was set
// by ivf_init_kernel)
static int ivf_group(const int64_t* probe, int64_t nq, int nprobe, int nlist, const int64_t* list_off, int wq, int ch,
                     int dp, int64_t max_rows, const uint16_t* qh, int* cnt, int* fill, int* seg, int* work, int* sp,
                     uint16_t* qi, int* H, int* err, hipStream_t st, bool fill_sp = true) {
  const int64_t npairs = nq * nprobe;
  if (fill_sp && hipMemsetAsync(sp, 0xff, (size_t)max_rows * 4, st) != hipSuccess)
    return fail(NRK_ELAUNCH, "ivf_search: memset failed");
  if (nlist <= GROUP_LDS_LISTS) {
    const size_t lds = (size_t)nlist * 4;
    hipLaunchKernelGGL(ivf_hist_kernel, dim3(GROUP_BLOCKS), dim3(1024), lds, st, probe, npairs, nlist, H);
    NRK_CHECK_LAUNCH("ivf_hist_kernel");
    hipLaunchKernelGGL(ivf_plan_kernel, dim3(1), dim3(1024), 0, st, cnt, list_off, nlist, wq, ch, seg, work, fill, H,
                       GROUP_BLOCKS);
    NRK_CHECK_LAUNCH("ivf_plan_kernel");
    hipLaunchKernelGGL(ivf_place_kernel, dim3(GROUP_BLOCKS), dim3(1024), lds, st, probe, npairs, nlist, seg, H, sp);
    NRK_CHECK_LAUNCH("ivf_place_kernel");
  } else {
    if (hipMemsetAsync(cnt, 0, (size_t)nlist * 4, st) != hipSuccess)
      return fail(NRK_ELAUNCH, "ivf_search: memset failed");
    hipLaunchKernelGGL(ivf_count_kernel, dim3((unsigned)cdiv(npairs, 256)), dim3(256), 0, st, probe, npairs, nlist,
                       cnt);
    NRK_CHECK_LAUNCH("ivf_count_kernel");
    hipLaunchKernelGGL(ivf_plan_kernel, dim3(1), dim3(1024), 0, st, cnt, list_off, nlist, wq, ch, seg, work, fill,
                       nullptr, 0);
    NRK_CHECK_LAUNCH("ivf_plan_kernel");
    hipLaunchKernelGGL(ivf_scatter_kernel, dim3((unsigned)cdiv(npairs, 256)), dim3(256), 0, st, probe, npairs, nlist,
                       seg, fill, sp);
    NRK_CHECK_LAUNCH("ivf_scatter_kernel");
  }
  const int64_t gblk = cdiv(max_rows, 4) < GATHER_BLOCKS ? cdiv(max_rows, 4) : GATHER_BLOCKS;
  hipLaunchKernelGGL(ivf_gather_kernel, dim3((unsigned)gblk), dim3(256), 0, st, qh, dp, nprobe, sp, seg,
                     nlist, max_rows, qi, npairs, err);
  NRK_CHECK_LAUNCH("ivf_gather_kernel");
  return NRK_OK;
}

}  // namespace nrk

using namespace nrk;

extern "C" int nrk_ivf_search_workspace(int64_t nq, int32_t nprobe, int32_t nlist, int64_t max_list, int32_t d,
                                        int32_t k, size_t* ws_bytes) {
  NRK_CHECK_ARG(ws_bytes && nq >= 0 && nprobe > 0 && nlist > 0 && max_list >= 0 && d > 0 && d <= 256 && k > 0 &&
                    k <= 256,
                "ivf_search_workspace: bad arguments");
  *ws_bytes = make_ivf_plan(nq, nprobe, nlist, max_list, d, k).total;
  return NRK_OK;
}

extern "C" int nrk_ivf_search(const float* xq, int64_t nq, const int64_t* probe, int32_t nprobe, const float* xb,
                              const uint16_t* xbh_ivf, const float* meta_ivf, const float* stats,
                              const int64_t* list_off, const int64_t* pos2id, const int32_t* pos2list, int32_t nlist,
                              int64_t n, int64_t max_list, int32_t d, int32_t k, int32_t metric, float* D, int64_t* I,
                              double* S, int64_t id_offset, int32_t* n_fallback, void* ws, size_t ws_bytes,
                              void* const* stage_events, void* stream) {
  NRK_CHECK_ARG(nq >= 0 && nprobe > 0 && nlist > 0 && n >= 0 && max_list >= 0 && d > 0 && d <= 256 && k > 0 &&
                    k <= 256,
                "ivf_search: bad shape nq=%lld nprobe=%d nlist=%d d=%d k=%d", (long long)nq, nprobe, nlist, d, k);
  NRK_CHECK_ARG(metric == NRK_METRIC_INNER_PRODUCT || metric == NRK_METRIC_L2, "ivf_search: bad metric %d", metric);
  NRK_CHECK_ARG(n < ((int64_t)1 << 31), "ivf_search: %lld rows exceed int32 positions", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  const IvfPlan p = make_ivf_plan(nq, nprobe, nlist, max_list, d, k);
  if (ws_bytes < p.total) return fail(NRK_EWORKSPACE, "ivf_search: workspace %zu < %zu bytes", ws_bytes, p.total);
  NRK_CHECK_ARG(ws != nullptr, "ivf_search: null workspace");
  NRK_CHECK_ARG(nq == 0 || (xq && probe && D && I && list_off), "ivf_search: null pointer");
  NRK_CHECK_ARG(n == 0 || (xb && xbh_ivf && meta_ivf && stats && pos2id && pos2list), "ivf_search: null index data");
  const int l2 = metric == NRK_METRIC_L2;
  auto mark = [&](int i) {
    if (stage_events) (void)hipEventRecord((hipEvent_t)stage_events[i], st);
  };
  IvfWs w;
  ivf_carve(static_cast<char*>(ws), p, nq, nlist, w);
  const FbState fb{w.fbl, w.fbc, p.fb_slots, p.fb_slots, w.fbt, w.fbi, w.fbn, 0};
  int* gerr = w.fbc + IVF_GUARD_INT;  // the guard word (zeroed with the counters; nrk_ivf_search_status)
  IvfFb ivf{pos2id, pos2list, list_off, probe, nprobe, nlist, nq, gerr};
  const bool force_fb = test_hook("NRK_FORCE_FALLBACK", 0) != 0;
  mark(0);
  {  // counters, guard word, n_fallback, candidate counts; with rows: phase A's p0 / pt / sp
    const bool rows = n > 0 && nq > 0;
    const int64_t npt = rows ? nq * p.nA * p.cmaxA * 2 : 0, nsp = rows ? p.max_rows : 0;
    int64_t big = npt > nsp ? npt : nsp;
    if (nq * p.nA > big) big = nq * p.nA;
    const unsigned gi = (unsigned)(big > 16 ? (cdiv(big, 256) < 2048 ? cdiv(big, 256) : 2048) : 1);
    hipLaunchKernelGGL(ivf_init_kernel, dim3(gi), dim3(256), 0, st, w.fbc, n_fallback, w.p0, probe, nq, rows ? nq : 0,
                       nprobe, p.nA, reinterpret_cast<uint32_t*>(w.pt), npt, w.ccnt, w.sp, nsp);
    NRK_CHECK_LAUNCH("ivf_init_kernel");
  }
  if (nq == 0) return NRK_OK;

  int rc = query_prepare_launch(xq, nq, p.nq_pad, d, p.dp, w.qh, w.qmeta, nullptr, nullptr, st);
  if (rc != NRK_OK) return rc;
  if (n > 0) {
    // ---- phase A: lane maxima over the nearest list of every query -> tau
    // (p0, pt (NaN: never selected), ccnt and sp were set by ivf_init_kernel)
    rc = ivf_group(w.p0, nq, p.nA, nlist, list_off, p.wqA, p.chA, p.dp, p.max_rows, w.qh, w.cnt, w.fill, w.seg, w.work,
                   w.sp, w.qi, w.hist, gerr, st, false);
    if (rc != NRK_OK) return rc;
    screen_fn fa = pick_screen(p.dp, p.qtA, p.M, l2 != 0, 4);
    if (!fa) return fail(NRK_EUNSUPPORTED, "ivf_search: no screen kernel for dp=%d", p.dp);
    IvfScreen isa{w.work, list_off, w.seg, w.sp, nlist, p.chA, p.cmaxA, nullptr, nullptr, nullptr, 0, p.nA, nullptr, gerr};
    hipLaunchKernelGGL(fa, dim3((unsigned)p.ubA), dim3(p.waves * 64), 0, st, w.qi, xbh_ivf, meta_ivf, nq, n, 0, 0, 0,
                       3, nullptr, w.pa, w.pt, nullptr, isa);  // every third tile: seeds from a third of the rows
    // (tile strides 2 / 3 / 4 / 6: search 3.49 / 3.46 / 3.48 / 3.50 ms, phase A falling and the
    // exact rescore of the wider collect rising; profiles/r04_ivf_phaseA_stride_ab.log)
    NRK_CHECK_LAUNCH("screen_kernel (ivf phase A)");
    const int nva = 2 * p.nA * p.cmaxA;
    hipLaunchKernelGGL(tau_select_fn(nva), dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, st, w.pt, nva, p.R, nq, w.tau,
                       w.pa, w.seed);
    NRK_CHECK_LAUNCH("tau_select_kernel (ivf)");
    hipLaunchKernelGGL(ivf_seed_kernel, dim3((unsigned)nq), dim3(64), (size_t)pow2ceil(p.R) * 16 + (size_t)d * 4, st,
                       w.seed, p.R, k, pos2id, xq, xb, d, l2, w.qmeta, stats, p.dp, w.thr, w.lbg, w.lbi, w.ccnt, p.cap,
                       n, gerr);
    NRK_CHECK_LAUNCH("ivf_seed_kernel");
    // ---- phase B grouping: every probed list
    rc = ivf_group(probe, nq, nprobe, nlist, list_off, p.wq, p.chB, p.dp, p.max_rows, w.qh, w.cnt, w.fill, w.seg,
                   w.work, w.sp, w.qi, w.hist, gerr, st);
    if (rc != NRK_OK) return rc;
  }  // (empty index: ccnt zeroed by ivf_init_kernel, so every query reads all -1)

  mark(1);
  if (n > 0) {
    // ---- phase B: collect every probed item at or above e_k - B_q
    screen_fn fbk = pick_screen(p.dp, p.qt, p.M, l2 != 0, 3);
    // the 16x16x32 collect where built (NRK_SCREEN16=0: the 32x32x16 one; a test hook)
    if (p.dp == 128 && p.qt == 2 && p.wavesB == 4 && test_hook("NRK_SCREEN16", 1)) fbk = pick_collect16_dp128(l2 != 0);
    if (!fbk) return fail(NRK_EUNSUPPORTED, "ivf_search: no collect kernel for dp=%d", p.dp);
    IvfScreen isb{w.work, list_off, w.seg, w.sp, nlist, p.chB, p.cmaxB, w.thr, w.ccnt, w.cpos, p.cap, nprobe,
                  w.fbc + 8, gerr};
    hipLaunchKernelGGL(fbk, dim3((unsigned)p.ubB), dim3(p.wavesB * 64), 0, st, w.qi, xbh_ivf, meta_ivf, nq, n, 0, 0, 0,
                       1, nullptr, nullptr, nullptr, nullptr, isb);
    NRK_CHECK_LAUNCH("screen_kernel (ivf collect)");
  }

  mark(2);
  if (force_fb && n > 0 && hipMemsetAsync(w.ccnt, 0x7f, (size_t)nq * 4, st) != hipSuccess)  // testing: overflow all
    return fail(NRK_ELAUNCH, "ivf_search: memset failed");
  rc = collect_rescore_launch((int)nq, w.ccnt, w.cpos, p.cap, pos2id, xq, xb, d, k, l2, w.lbg, w.lbi, D, I, S, id_offset,
                              fb, nq, n, gerr, nullptr, nullptr, st);
  if (rc != NRK_OK) return rc;

  mark(3);
  rc = fallback_tail(xq, nq, xb, n, d, k, l2, fb, w.fcg, w.fci, p.fb_cap, w.ovl, D, I, S, id_offset, ivf, st);
  if (rc != NRK_OK) return rc;
  mark(4);
  // [0] the tiled fp64 scan's queries (collect overflow / too few seeds), [1] of
  // those, the ones its buffer could not hold either (the block-per-query scan)
  if (n_fallback && hipMemcpyAsync(n_fallback, w.fbc, 8, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(NRK_ELAUNCH, "ivf_search: copy of fallback counts failed");
  return NRK_OK;
}

// The guard word of the last nrk_ivf_search on this workspace (GuardCode bits,
// 0 = every workspace-derived index was in range) -> device int32 (async).
extern "C" int nrk_ivf_search_status(const void* ws, size_t ws_bytes, int32_t* guard, void* stream) {
  NRK_CHECK_ARG(ws != nullptr && guard != nullptr && ws_bytes >= 64, "ivf_search_status: bad arguments");
  if (hipMemcpyAsync(guard, static_cast<const char*>(ws) + IVF_GUARD_BYTE, 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
      hipSuccess)
    return fail(NRK_ELAUNCH, "ivf_search_status: copy failed");
  return NRK_OK;
}

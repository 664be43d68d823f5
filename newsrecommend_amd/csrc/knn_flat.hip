// knn_flat.hip — exact flat k-NN for gfx950 (replaces faiss IndexFlatIP /
// IndexFlatL2 .search, Retrieval.py:21,25-32).
//
// Pipeline per search (all on the caller's stream, no host sync):
//   1. query_prepare  : xq -> bf16 q^ (zero-padded to DP), per-query norms
//   2. screen         : bf16 MFMA (32x32x16) query x corpus-chunk tiles; every
//                       lane keeps its top-(M+1) screened scores in registers;
//                       writes M candidates + the (M+1)-th score (theta) per
//                       (query, chunk, lane-half)
//   3. merge_rescore  : per query: select the top KP of the union of candidates,
//                       rescore them EXACTLY (fp64, sequential d —
//                       bit-identical to oracle/knn_exact.c), sort, and certify
//                       with a rigorous screening error bound that no item
//                       outside the KP candidates can enter the exact top-k;
//                       uncertified queries are appended to a fallback list
//   4. collect pass   : the uncertified queries (normally none) screened again,
//                       every item within the bound rescored exactly
//   5. fallback_tail  : fp64 scans for what is left (knn_exact.hip)
// Small and unplannable shapes go straight to knn_exact.hip's fp64 paths.
// See DESIGN.md "K-GEMM-TOPK" for the bound and the roofline.
#include "knn_common.h"
#include "screen16.h"

namespace nrk {

// ================================================================ prepare ==
// One wave per row, grid-stride; the three corpus maxima are reduced per wave
// and published with one atomic each (per-row atomics on three addresses
// serialise at the L2).
__global__ void flat_prepare_kernel(const float* __restrict__ xb, int64_t nb, int d, int dp,
                                    uint16_t* __restrict__ xbh, float* __restrict__ meta,
                                    float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  float m0 = 0.f, m1 = 0.f, m2 = 0.f;
  for (int64_t row = wave0; row < nb; row += nwaves) {
    double sx2 = 0.0, sh2 = 0.0, sr2 = 0.0;
    for (int j = lane; j < dp; j += 64) {
      float x = j < d ? xb[row * d + j] : 0.f;
      uint16_t h = f32_to_bf16_rne(x);
      float hf = bf16_to_f32(h);
      double r = (double)x - (double)hf;
      sx2 += (double)x * (double)x;
      sh2 += (double)hf * (double)hf;
      sr2 += r * r;
      xbh[row * dp + j] = h;
    }
    sx2 = wave_sum(sx2);
    sh2 = wave_sum(sh2);
    sr2 = wave_sum(sr2);
    const float rn = f64_to_f32_up(sqrt(sr2) * (1.0 + 1e-9));
    if (lane == 0) {
      meta[2 * row] = (float)sx2;
      meta[2 * row + 1] = rn;
    }
    m0 = fmaxf(m0, f64_to_f32_up(sqrt(sh2) * (1.0 + 1e-9)));
    m1 = fmaxf(m1, rn);
    m2 = fmaxf(m2, f64_to_f32_up(sx2 * (1.0 + 1e-9)));
  }
  if (lane == 0 && wave0 < nb) {
    atomic_max_nonneg(&stats[0], m0);
    atomic_max_nonneg(&stats[1], m1);
    atomic_max_nonneg(&stats[2], m2);
  }
}

// qmeta[4*q] = {||q^|| (up), ||q - q^|| (up), ||q||^2, 0}
__global__ void query_prepare_kernel(const float* __restrict__ xq, int64_t nq, int64_t nq_pad, int d,
                                     int dp, uint16_t* __restrict__ qh, double* __restrict__ qmeta,
                                     int* __restrict__ zero4, int* __restrict__ zero2) {
  const int lane = threadIdx.x & 63;
  // the search's fallback counters (instead of two memset launches)
  if (blockIdx.x == 0 && threadIdx.x < 4 && zero4) zero4[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x < 2 && zero2) zero2[threadIdx.x] = 0;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= nq_pad) return;
  double sq2 = 0.0, sh2 = 0.0, sr2 = 0.0;
  for (int j = lane; j < dp; j += 64) {
    float x = (row < nq && j < d) ? xq[row * d + j] : 0.f;
    uint16_t h = f32_to_bf16_rne(x);
    float hf = bf16_to_f32(h);
    double r = (double)x - (double)hf;
    sq2 += (double)x * (double)x;
    sh2 += (double)hf * (double)hf;
    sr2 += r * r;
    qh[row * dp + j] = h;
  }
  sq2 = wave_sum(sq2);
  sh2 = wave_sum(sh2);
  sr2 = wave_sum(sr2);
  if (lane == 0 && row < nq) {
    qmeta[4 * row + 0] = sqrt(sh2) * (1.0 + 1e-9);
    qmeta[4 * row + 1] = sqrt(sr2) * (1.0 + 1e-9);
    qmeta[4 * row + 2] = sq2;
    qmeta[4 * row + 3] = 0.0;
  }
}

int query_prepare_launch(const float* xq, int64_t nq, int64_t nq_pad, int d, int dp, uint16_t* qh, double* qmeta,
                         int* zero4, int* zero2, hipStream_t st) {
  hipLaunchKernelGGL(query_prepare_kernel, dim3((unsigned)cdiv(nq_pad, 4)), dim3(256), 0, st, xq, nq, nq_pad, d, dp, qh,
                     qmeta, zero4, zero2);
  NRK_CHECK_LAUNCH("query_prepare_kernel");
  return NRK_OK;
}

// tau[q] = the R-th largest finite lane maximum of the pre-pass (or -inf if
// there are fewer than R): R distinct items score at least this much, so it
// never exceeds the query's global R-th best screened score.  One wave per
// query, values in registers.  Exact selection by bisection on the ordered
// integer keys of the floats (32 rounds of ballot counts), not R rounds of
// wave argmax (k = 200: R = 400 rounds took 0.33 ms per 4096 queries).
//
// With ids_in (IVF phase A: the position of each lane maximum), ids_out[q][i]
// receives the positions of R entries >= tau (all above it, then ties in
// (value slot, lane) order), or of every finite entry (-1 past the end).
//
// VPL: values per lane (nvals <= 64 * VPL); the flat pre-pass writes 8R = 64
// values per query for k <= 8, so VPL = 1 there (16x fewer ballots per
// bisection round than the VPL = 16 form)
template <int VPL>
__global__ __launch_bounds__(256) void tau_select_kernel(const float* __restrict__ premax, int nvals, int R,
                                                         int64_t nq, float* __restrict__ tau,
                                                         const int* __restrict__ ids_in,
                                                         int* __restrict__ ids_out) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  if (ids_out)
    for (int i = lane; i < R; i += 64) ids_out[q * R + i] = -1;
  uint32_t key[VPL];       // 0: not finite (-inf, NaN: never selected)
  int nfin = 0;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int i = j * 64 + lane;
    const float v = i < nvals ? premax[q * nvals + i] : -INFINITY;
    key[j] = v > -INFINITY ? ordered_key(v) : 0u;
    nfin += __popcll(__ballot(key[j] != 0u));
  }
  const uint32_t K = nfin >= R ? wave_kth_key(key, R) : 0u;  // (0: fewer than R finite values)
  if (lane == 0) tau[q] = K ? key_value(K) : -INFINITY;
  if (!ids_out) return;
  wave_take_top(key, K, R, [&](int j, int pos) {
    if (pos < R) ids_out[q * R + pos] = ids_in[q * nvals + j * 64 + lane];
  });
}

tau_select_fn_t tau_select_fn(int nvals) {
  return nvals <= 64 ? tau_select_kernel<1> : nvals <= 256 ? tau_select_kernel<4>
       : nvals <= 512 ? tau_select_kernel<8> : tau_select_kernel<16>;
}

// ========================================================= merge/rescore ==
// Top-kp selection for merge_rescore_kernel (256 threads, EPT union entries
// per thread in registers): the kp best by screened score -> ids[0, kp)
// (unordered; ids[kp, P2) = INT64_MAX), by a bisection on the order-preserving
// keys of the float scores instead of a bitonic sort of the union.  Returns the
// best score left out.
//
// A union of at most 64 NK entries (U <= 1024): the
// keys and ids go to LDS, then wave 0 alone runs the bisection with wave
// ballots over NK keys per lane (no block barrier per round); ties at the cut
// are taken in slot order (deterministic; any choice keeps the certificate,
// which bounds every left-out item by the best left-out score, returned).
template <int NK, int EPT>
__device__ float select_top_wave(const double* rg, const int64_t* ri, const bool* rv, int U, int kp,
                                 uint32_t* kbuf, int64_t* ibuf, int64_t* ids, int P2) {
  __shared__ float s_out;
  const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + 256 * e;
    if (i < U) {
      kbuf[i] = rv[e] ? ordered_key((float)rg[e]) : 0u;  // valid keys are >= 1
      ibuf[i] = ri[e];
    }
  }
  __syncthreads();
  if (tid < 64) {
    uint32_t kk[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) kk[j] = lane + 64 * j < U ? kbuf[lane + 64 * j] : 0u;
    const uint32_t T = wave_kth_key(kk, kp);  // (>= 1: more than kp entries are valid)
    uint32_t kout = wave_take_top(kk, T, kp, [&](int j, int pos) { ids[pos] = ibuf[lane + 64 * j]; });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kout = max(kout, (uint32_t)__shfl_xor((int)kout, o, 64));
    if (lane == 0) s_out = kout ? key_value(kout) : -INFINITY;
  }
  for (int i = kp + tid; i < P2; i += 256) ids[i] = INT64_MAX;
  __syncthreads();
  return s_out;
}

// Larger unions: 32 block counts; ties at the cut are taken by ascending id.
// g / id (the union's LDS) are scratch.
template <int EPT>
__device__ float select_top(const double* rg, const int64_t* ri, const bool* rv, int kp, double* g, int64_t* id,
                            int64_t* ids, int P2) {
  __shared__ int cnt[2][4], csum[4];
  __shared__ uint32_t kmax[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t key[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) key[e] = rv[e] ? ordered_key((float)rg[e]) : 0u;  // valid keys are >= 1
  auto block_count = [&](uint32_t c, bool strict, int buf) {
    int n = 0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) n += __popcll(__ballot(strict ? key[e] > c : key[e] >= c));
    if (lane == 0) cnt[buf][w] = n;
    __syncthreads();
    return cnt[buf][0] + cnt[buf][1] + cnt[buf][2] + cnt[buf][3];
  };
  uint32_t T = 0;  // the kp-th largest key
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t c = T | (1u << bit);
    if (block_count(c, false, bit & 1) >= kp) T = c;
  }
  const int ngt = block_count(T, true, 1);  // (buffer 1: last written two barriers ago)
  const int nge = block_count(T, false, 0);
  const int r = kp - ngt;  // ties at T to take (>= 1)
  // the id cut among the ties: all of them, or the r smallest ids
  int64_t idcut = INT64_MAX;
  if (nge - ngt > r) {
    __shared__ int nt;
    if (tid == 0) nt = 0;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPT; ++e)
      if (key[e] == T) {
        const int o = atomicAdd(&nt, 1);
        g[o] = 0.0;
        id[o] = ri[e];
      }
    __syncthreads();
    const int n2 = nt, P = pow2ceil(n2);
    for (int i = n2 + tid; i < P; i += 256) {
      g[i] = 0.0;
      id[i] = INT64_MAX;
    }
    __syncthreads();
    block_bitonic_sort(g, id, P);  // equal scores: ascending id
    idcut = id[r - 1];
    __syncthreads();
  }
  // compaction of the selected entries into ids[0, kp); the best key left out
  int ns = 0;
  uint32_t kout = 0;
  bool sel[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    sel[e] = key[e] > T || (key[e] == T && ri[e] <= idcut);
    ns += sel[e] ? 1 : 0;
    if (!sel[e] && rv[e]) kout = max(kout, key[e]);
  }
  int incl = ns;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kout = max(kout, (uint32_t)__shfl_xor((int)kout, o, 64));
  if (lane == 63) csum[w] = incl;
  if (lane == 0) kmax[w] = kout;
  __syncthreads();
  int off = incl - ns;
  for (int j = 0; j < w; ++j) off += csum[j];
#pragma unroll
  for (int e = 0; e < EPT; ++e)
    if (sel[e]) ids[off++] = ri[e];
  for (int i = kp + tid; i < P2; i += 256) ids[i] = INT64_MAX;
  const uint32_t km = max(max(kmax[0], kmax[1]), max(kmax[2], kmax[3]));
  __syncthreads();
  return km ? key_value(km) : -INFINITY;
}

// One 256-thread workgroup per query.  Dynamic LDS: P doubles + P int64 (the
// union's valid ids and the selection's scratch; later the rescoring's row
// stage, at least 256 x (RS_CW + 4) floats), P2 doubles + P2 int64 (rescored),
// d floats (query), reductions.
constexpr int RS_CW = 32;       // columns per rescoring stage (one 128-B line of each candidate row)
constexpr int RS_MIN_KP = 128;  // staged rescoring from this many candidates (k = 5: lane-per-row loads)
// bytes of the merge's union region: the union (P doubles + P ids), the
// rescoring stage, or the small selection's 256 keys + 256 ids
__host__ __device__ inline int merge_union_bytes(int P, int KP) {
  int ub = 16 * P;
  if (KP >= RS_MIN_KP && ub < 256 * (RS_CW + 4) * 4) ub = 256 * (RS_CW + 4) * 4;
  if (ub < 12 * P + 16) ub = 12 * P + 16;  // the wave selection: P keys + P ids (P >= U)
  return ub;
}
__global__ __launch_bounds__(256) void merge_rescore_kernel(
    const float* __restrict__ part_s, const int* __restrict__ part_i, const float* __restrict__ part_t,
    int nch, int M, int KP, int k, int dp, const float* __restrict__ xq, const float* __restrict__ xb,
    int64_t nb, int d, int l2, const double* __restrict__ qmeta, const float* __restrict__ stats,
    const float* __restrict__ tau_q, float* __restrict__ D, int64_t* __restrict__ I, double* __restrict__ S,
    int64_t id_offset, FbState fb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int qi = blockIdx.x, tid = threadIdx.x;
  const int U = nch * 2 * M, P = pow2ceil(U);
  double* g = reinterpret_cast<double*>(smem);
  int64_t* id = reinterpret_cast<int64_t*>(g + P);
  const int P2 = pow2ceil(KP);
  const int UB = merge_union_bytes(P, KP);  // union / stage / small selection
  double* g2 = reinterpret_cast<double*>(smem + UB);
  int64_t* id2 = reinterpret_cast<int64_t*>(g2 + P2);
  float* qs = reinterpret_cast<float*>(id2 + P2);
  __shared__ float red[256];

  const float* ps = part_s + (int64_t)qi * U;
  const int* pi = part_i + (int64_t)qi * U;
  // the union (U <= 2048: at most 8 entries per thread) -> registers; only the
  // valid entries (with the pre-pass bound: a few hundred at k = 200, of 2048)
  // are compacted to the front
  constexpr int EPT = 8;
  double rg[EPT];
  int64_t ri[EPT];
  bool rv[EPT];
  int nv = 0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + 256 * e;
    const float v = i < U ? ps[i] : -INFINITY;
    const int64_t item = i < U ? (int64_t)pi[i] : -1;
    rv[e] = v != -INFINITY && item >= 0 && item < nb;  // never dereference an unset slot
    rg[e] = (double)v;
    ri[e] = rv[e] ? item : INT64_MAX;
    nv += rv[e] ? 1 : 0;
  }
  const int lane = tid & 63, w = tid >> 6;
  int incl = nv;  // inclusive prefix of the valid counts within the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __shared__ int wsum[4];
  if (lane == 63) wsum[w] = incl;
  float th = -INFINITY;
  for (int i = tid; i < nch * 2; i += 256) th = fmaxf(th, part_t[(int64_t)qi * nch * 2 + i]);
  red[tid] = th;
  for (int i = tid; i < d; i += 256) qs[i] = xq[(int64_t)qi * d + i];
  __syncthreads();
  const int V = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  int off = incl - nv;
  for (int j = 0; j < w; ++j) off += wsum[j];
#pragma unroll
  for (int e = 0; e < EPT; ++e)
    if (rv[e]) id[off++] = ri[e];
  const bool staged = (d & 3) == 0 && KP >= RS_MIN_KP;  // many candidates: rows staged through LDS
  for (int o = 128; o > 0; o >>= 1) {  // (its first barrier also publishes the compaction)
    __syncthreads();
    if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
  }
  __syncthreads();
  const float theta_lanes = red[0];
  const int kp = KP < V ? KP : V;
  double theta = theta_lanes;
  // the top kp are SELECTED, not sorted (the exact scores are sorted afterwards)
  if (kp < V) {
    uint32_t* kb = reinterpret_cast<uint32_t*>(smem);
    int64_t* ib = reinterpret_cast<int64_t*>(smem + 4 * P);
    const float left = U <= 256 ? select_top_wave<4, EPT>(rg, ri, rv, U, kp, kb, ib, id2, P2)
                       : U <= 512 ? select_top_wave<8, EPT>(rg, ri, rv, U, kp, kb, ib, id2, P2)
                       : U <= 1024 ? select_top_wave<16, EPT>(rg, ri, rv, U, kp, kb, ib, id2, P2)
                                   : select_top<EPT>(rg, ri, rv, kp, g, id, id2, P2);
    theta = fmax(theta, (double)left);
  } else {
    for (int i = tid; i < P2; i += 256) id2[i] = i < kp ? id[i] : INT64_MAX;
    __syncthreads();
  }
  if (tau_q) theta = fmax(theta, (double)tau_q[qi]);  // items below the bound were never kept

  // exact rescoring of the top kp screened candidates
  if (staged) {
    // the union's LDS is the stage (its ids moved to id2)
    staged_rescore<RS_CW>(reinterpret_cast<float*>(smem), id2, kp, xb, d, qs, l2, g2);
    for (int i = kp + tid; i < P2; i += 256) g2[i] = -INFINITY;
  } else {
    for (int i = tid; i < P2; i += 256) {
      if (i < kp) {
        const double s = exact_score(qs, xb + id2[i] * d, d, l2 != 0);
        g2[i] = l2 ? -s : s;
      } else {
        g2[i] = -INFINITY;
        id2[i] = INT64_MAX;
      }
    }
  }
  __syncthreads();
  block_bitonic_sort(g2, id2, P2);

  if (tid == 0) {
    bool ok = kp >= k;
    if (ok && theta != -INFINITY) {
      const double nqh = qmeta[4 * qi + 0], nrq = qmeta[4 * qi + 1], qn2 = qmeta[4 * qi + 2];
      const double Xh = stats[0], R = stats[1], NX = stats[2];
      const double gam = (double)dp * 0x1p-22;
      const double bip = gam * nqh * Xh + nqh * R + nrq * Xh + nrq * R;
      const double kth = g2[k - 1];
      if (!l2) {
        const double lim = theta + bip;
        ok = kth - lim > 1e-12 * (fabs(lim) + fabs(kth));
      } else {
        const double B = 2.0 * bip + 0x1p-21 * (NX + nqh * Xh);
        const double lo = qn2 - theta - B;  // lower bound on any outsider's distance
        ok = lo - (-kth) > 1e-12 * (fabs(lo) + fabs(kth) + qn2);
      }
    }
    if (fb.force) ok = false;
    if (!ok) fb.push(qi, kp >= k ? g2[k - 1] : -INFINITY, kp >= k ? id2[k - 1] : (int64_t)-1);
  }
  for (int j = tid; j < k; j += 256) write_result(D, I, S, (int64_t)qi * k + j, j < kp, g2[j], id2[j], l2, id_offset);
}

// ======================================================== collect rescore ==
// The second half of a collect pass (IVF phase B, flat collect pass): exact
// rescoring of every collected candidate, top-k.  Queries whose buffer
// overflowed go to the fallback with threshold (e_k, id).
constexpr int CR_CW = 16;   // collect_rescore: columns per staging step
constexpr int CR_MIN = 64;  // ... staged from this many candidates
// dynamic LDS of collect_rescore_kernel for a candidate capacity and dimension
static size_t collect_rescore_smem(int cap, int d) {
  return (size_t)pow2ceil(cap) * 16 + (size_t)((d + 3) & ~3) * 4 + (size_t)256 * (CR_CW + 4) * 4;
}

__global__ __launch_bounds__(256) void collect_rescore_kernel(
    const int* __restrict__ cand_cnt, const int* __restrict__ cand_pos, int cap, const int64_t* __restrict__ pos2id,
    const float* __restrict__ xq, const float* __restrict__ xb, int d, int k, int l2,
    const double* __restrict__ lb_g, const int64_t* __restrict__ lb_i, float* __restrict__ D,
    int64_t* __restrict__ I, double* __restrict__ S, int64_t id_offset, FbState fb, int64_t nq, int64_t n,
    int* __restrict__ err, const int* __restrict__ qlist, const int* __restrict__ qcount) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  // IVF: slot = query.  Flat collect pass: slot b holds query qlist[b], if any.
  const int sl = blockIdx.x;
  if (qlist && sl >= *qcount) return;
  const int qi = qlist ? qlist[sl] : sl;
  if (!guard_ok((uint64_t)qi < (uint64_t)nq, err, GUARD_FB_QUERY)) return;
  int c = cand_cnt[sl];
  if (!guard_ok(c >= 0, err, GUARD_CAND_COUNT)) c = 0;
  if (c > cap) {
    if (tid == 0) fb.push(qi, lb_g[sl], lb_i[sl]);
    return;
  }
  const int P = pow2ceil(c > 0 ? c : 1);
  double* g = reinterpret_cast<double*>(smem);
  int64_t* id = reinterpret_cast<int64_t*>(g + P);
  float* qs = reinterpret_cast<float*>(id + P);
  for (int i = tid; i < d; i += 256) qs[i] = xq[(int64_t)qi * d + i];
  const bool staged = (d & 3) == 0 && c >= CR_MIN;
  for (int i = tid; i < P; i += 256) {
    if (i < c) {
      const int pos = cand_pos[(int64_t)sl * cap + i];
      // an out-of-range position (a broken invariant) is flagged and read as row 0
      const int64_t p = guard_ok((uint64_t)pos < (uint64_t)n, err, GUARD_CAND_POS) ? pos : 0;
      id[i] = pos2id ? pos2id[p] : p;
    } else {
      g[i] = -INFINITY;
      id[i] = INT64_MAX;
    }
  }
  __syncthreads();
  if (staged) {
    staged_rescore<CR_CW>(qs + ((d + 3) & ~3), id, c, xb, d, qs, l2, g);
  } else {
    for (int i = tid; i < c; i += 256) {
      const double sc = exact_score(qs, xb + id[i] * d, d, l2 != 0);
      g[i] = l2 ? -sc : sc;
    }
  }
  __syncthreads();
  block_bitonic_sort(g, id, P);
  for (int j = tid; j < k; j += 256) {
    const bool valid = j < c;  // (j may lie past the sorted P entries)
    write_result(D, I, S, (int64_t)qi * k + j, valid, valid ? g[j] : 0.0, valid ? id[j] : 0, l2, id_offset);
  }
}

int collect_rescore_launch(int nslots, const int* cand_cnt, const int* cand_pos, int cap, const int64_t* pos2id,
                           const float* xq, const float* xb, int d, int k, int l2, const double* lb_g,
                           const int64_t* lb_i, float* D, int64_t* I, double* S, int64_t id_offset, FbState fb,
                           int64_t nq, int64_t n, int* err, const int* qlist, const int* qcount, hipStream_t st) {
  hipLaunchKernelGGL(collect_rescore_kernel, dim3((unsigned)nslots), dim3(256), collect_rescore_smem(cap, d), st,
                     cand_cnt, cand_pos, cap, pos2id, xq, xb, d, k, l2, lb_g, lb_i, D, I, S, id_offset, fb, nq, n, err,
                     qlist, qcount);
  NRK_CHECK_LAUNCH("collect_rescore_kernel");
  return NRK_OK;
}

// ====================================================== flat collect pass ==
// Queries the flat merge could not certify (dense neighbourhoods: the exact
// k-th best lies within the screening error bound of theta) get a second,
// exact-by-construction pass instead of an fp64 corpus scan: the IVF collect
// screen (MODE 3) over the whole corpus as ONE list, probed only by these
// queries, appends every item whose screened score reaches the query's collect
// threshold (from the merge's exact k-th e_k, collect_threshold), and
// collect_rescore ranks the candidates exactly.  Only a buffer overflow (more
// than `cap` items within the bound) goes on to the tiled fp64 fallback.
//
// Collect storage is indexed by slot s: round r of the pass takes the merge's
// fallback entries [r S, r S + S) (S = FB_SLOTS_MAX; every entry carries the
// merge's e_k), so any number of uncertified queries is collected in
// ceil(nq / S) rounds over the same fixed storage (a search of N x 4096
// queries against one corpus shard leaves more than S uncertified at L2).
// One block: turns this round's entries into the one-list work table
// (list_off, seg_off, work_off, slot_pair = s), the per-slot thresholds and
// the gathered bf16 query rows, and saves the slot -> query map for
// collect_rescore.  Queries whose candidates overflow the collect buffer go to
// the tiled fallback's own list (collect_rescore pushes them there).
__global__ __launch_bounds__(1024) void flat_collect_plan_kernel(
    FbState fb, int64_t nq, int64_t nb, int wq, int ch, const double* __restrict__ qmeta,
    const float* __restrict__ stats, int dp, int l2, int cap, int force_overflow, int round, int S,
    int64_t* __restrict__ list_off, int* __restrict__ seg_off, int* __restrict__ work_off, int* __restrict__ slot_pair,
    float* __restrict__ thr, double* __restrict__ lb_g, int64_t* __restrict__ lb_i, int* __restrict__ cand_cnt,
    int* __restrict__ clist, int* __restrict__ ccount, const uint16_t* __restrict__ qh, uint16_t* __restrict__ qc) {
  const int t = threadIdx.x, nt = blockDim.x;
  const int n = (int)min((int64_t)fb.count[0], nq);
  const int lo = round * S;
  const int nc = n - lo <= 0 ? 0 : (n - lo < S ? n - lo : S);  // this round's slots
  const int rows = (nc + wq - 1) / wq * wq;
  for (int s = t; s < rows; s += nt) slot_pair[s] = s < nc ? s : -1;
  for (int s = t; s < nc; s += nt) {
    const int q = fb.list[lo + s];
    clist[s] = q;
    const bool has = fb.thr_i[lo + s] >= 0;  // the merge rescored >= k candidates
    thr[s] = has ? collect_threshold(fb.thr_g[lo + s], qmeta + 4 * q, stats, dp, l2) : INFINITY;
    lb_g[s] = has ? fb.thr_g[lo + s] : -INFINITY;
    lb_i[s] = has ? fb.thr_i[lo + s] : -1;
    cand_cnt[s] = (has && !force_overflow) ? 0 : cap + 1;
  }
  if (t == 0) {
    list_off[0] = 0;
    list_off[1] = nb;
    seg_off[0] = 0;
    seg_off[1] = rows;
    work_off[0] = 0;
    work_off[1] = rows / wq * (int)cdiv(nb, (int64_t)ch);
    ccount[0] = nc;
    ccount[1] = n;  // queries the certificate did not cover (reported as n_fallback[0])
  }
  // the collected slots' bf16 query rows (padding rows zero): one wave per row
  for (int row = t >> 6; row < rows; row += nt >> 6) {
    const int64_t q = row < nc ? fb.list[lo + row] : -1;
    for (int j = (t & 63) * 4; j < dp; j += 256) {
      uint2 v = make_uint2(0u, 0u);
      if (q >= 0) v = *reinterpret_cast<const uint2*>(qh + q * dp + j);
      *reinterpret_cast<uint2*>(qc + (int64_t)row * dp + j) = v;
    }
  }
}

// ================================================================== plan ==
struct FlatPlan {
  bool exact_only, tau;
  bool cliff;  // exact_only forced by a shape the screen cannot plan (reported as nq fallbacks)
  bool small;  // nb <= SMALL_NB: exact fp64 tile GEMM (small_launch, geometry in sm)
  SmallPlan sm;
  int dp, qt, M, waves, wq, nqt, nch, U, KP;
  int pre_waves, nqt_pre;     // threshold pre-pass: waves per workgroup, query tiles (its own tile size)
  int R, nch_pre, tstride;  // threshold pre-pass: bound rank, chunks, tile stride
  int fb_slots, fb_cap;     // tiled fallback: slots with candidate storage, candidates per slot
  int64_t nq_pad, chunk, chunk_pre;
  size_t total;             // workspace bytes (flat_carve)
  // collect pass for uncertified queries (flat_collect_plan_kernel)
  int cwq, cch, ccap, cgrid;
  int64_t crows;
};

// The screened search's workspace, one line per region: type and element
// count, in workspace order, each region aligned to 256 B.  (The counters come
// first: the unscreened paths use them alone, at the workspace's base.)
struct FlatWs {
  int* fbc;          // [0] uncertified queries, [1] block-per-query scans, [2] tiled-fallback slots
  float *tau, *pre;  // pre-pass: bound per query, lane maxima
  uint16_t* qh;      // bf16 queries, padded
  double* qmeta;
  float* ps;         // main pass: lane lists (scores, items), (M+1)-th scores
  int* pi;
  float* pt;
  int* fbl;          // the merge's uncertified queries, their e_k (goodness, id)
  double* fbt;
  int64_t* fbi;
  int* fbn;          // tiled fallback: candidates seen / stored per slot
  double* fcg;
  int64_t* fci;
  int* ovl;          // queries for the block-per-query scan
  int* tfl;          // the tiled fallback's own list (collect buffer overflowed) and thresholds
  double* tft;
  int64_t* tfi;
  // collect pass: the one-list work table, then per-slot state
  int64_t* clo;
  int *cseg, *cwork, *csp;
  uint16_t* cqi;
  float* cthr;
  double* clbg;
  int64_t* clbi;
  int *ccnt, *cpos, *clist, *ccount;
};
static size_t flat_carve(char* base, const FlatPlan& p, int64_t nq, FlatWs& w) {
  Carver c{base};
  const size_t n = (size_t)nq, slots = (size_t)p.fb_slots;
  w.fbc = c.take<int>(4);
  w.tau = c.take<float>(n);
  w.pre = c.take<float>(n * p.nch_pre * 2);
  w.qh = c.take<uint16_t>((size_t)p.nq_pad * p.dp);
  w.qmeta = c.take<double>(n * 4);
  w.ps = c.take<float>(n * p.U);
  w.pi = c.take<int>(n * p.U);
  w.pt = c.take<float>(n * p.nch * 2);
  w.fbl = c.take<int>(n);
  w.fbt = c.take<double>(n);
  w.fbi = c.take<int64_t>(n);
  w.fbn = c.take<int>(slots);
  w.fcg = c.take<double>(slots * p.fb_cap);
  w.fci = c.take<int64_t>(slots * p.fb_cap);
  w.ovl = c.take<int>(n);
  w.tfl = c.take<int>(n);
  w.tft = c.take<double>(slots);
  w.tfi = c.take<int64_t>(slots);
  w.clo = c.take<int64_t>(2);
  w.cseg = c.take<int>(2);
  w.cwork = c.take<int>(2);
  w.csp = c.take<int>((size_t)p.crows);
  w.cqi = c.take<uint16_t>((size_t)p.crows * p.dp);
  w.cthr = c.take<float>(slots);
  w.clbg = c.take<double>(slots);
  w.clbi = c.take<int64_t>(slots);
  w.ccnt = c.take<int>(slots);
  w.cpos = c.take<int>(slots * p.ccap);
  w.clist = c.take<int>(slots);
  w.ccount = c.take<int>(4);
  return c.off;
}

// query count from which the DP = 128 inner-product main pass runs 512-query workgroups
// (screen ms, 4 vs 8 waves in one process at 1M x 128, k = 5: 512 queries 0.122 vs
// 0.122, 1024 0.226 vs 0.231, 2048 0.413 vs 0.413, 4096 0.783 vs 0.774)
constexpr int64_t W8_MIN_NQ = 4096;

static FlatPlan make_plan(int64_t nq, int64_t nb, int d, int k, bool l2) {
  FlatPlan p;
  memset(&p, 0, sizeof(p));
  p.dp = padded_dim(d);
  if (nb <= SMALL_NB && k <= SMALL_NB && nq > 0) {  // exact fp64 tile GEMM, no screening
    p.small = true;
    p.exact_only = true;
    p.sm = make_small_plan(nq, nb, k);
    p.total = p.sm.ws_bytes;
    return p;
  }
  p.exact_only = nb < EXACT_BELOW || d > 256 || k > 256 || nb >= (1ll << 31) || nq == 0;
  if (p.exact_only) {
    p.total = 256;  // the counters
    return p;
  }
  p.waves = 4;
  // M: per-lane list length.  tau: sampled pre-pass bound on the R-th best
  // screened score (R > k with margin), used while R stays small.
  if (k <= 8) { p.M = 4; p.qt = 2; }
  else if (k <= 24) { p.M = 8; p.qt = 1; }
  else { p.M = 16; p.qt = 1; }
  // DP = 256 with M = 4 or 16: 8-wave workgroups (256 queries per corpus pass):
  // half the LDS-DMA pieces per MFMA of the 4-wave form (10M x 256, k = 5:
  // screen 17.4 -> 15.0 ms) and, at k = 200, a chunk far larger than L2
  // re-read by half as many query tiles
  if (p.dp == 256 && (p.M == 4 || p.M == 16)) p.waves = 8;
  // DP = 128, M = 4, inner product (the 16x16x32 form): 8-wave workgroups of 512
  // queries, one per CU, from W8_MIN_NQ queries on (below 512 half a workgroup
  // scans zero rows).  One staged tile serves twice the queries: half the
  // LDS-DMA pieces per MFMA.  The pre-pass keeps its 4-wave kernel.
  if (p.dp == 128 && p.M == 4 && !l2 && test_hook("NRK_SCREEN16", 1)) {
    const int force = test_hook("NRK_SCREEN_WAVES", 0);
    if (force == 8 || (force != 4 && nq >= W8_MIN_NQ)) p.waves = 8;
  }
  // R: tau bounds the R-th best screened score from the pre-pass's lane maxima
  // (every stride-th tile), so it sits near global rank ~stride * R; the main
  // pass then admits ~stride * R items per query (list insertions, the VALU
  // cost of the k = 200 screen).  k > 8: R = k / 4 and stride * R >= 4k (below
  // that a few queries per thousand are uncertified: 1M x 128 k = 100 at 2k:
  // 36 of 4096).  Measured at 10M x 256 k = 200 (stride 16): screen 19.05 ms at
  // R = 2k -> 16.83; 1.25M x 256, 32768 queries: total 38.4 -> 29.2 ms.
  // k <= 8: R = max(8, k + 3) (was 16; with the stride rule below it halves the
  // pre-pass and leaves stride * R, the admitted items, unchanged: 1M x 128
  // k = 5 total 1.055 -> 1.001 ms, L2 1.41 -> 1.27 ms, 10M x 256 16.66 -> 16.41
  // ms, 125K x 128 x 32768 queries 1.78 -> 1.64 ms; same results).
  p.R = k <= 8 ? (k + 3 > 8 ? k + 3 : 8) : (k / 4 > 16 ? k / 4 : 16);
  p.tau = true;  // k = 200 at 10M x 256: -5% retrieve time
  if (p.dp == 256) p.qt = 1;
  p.wq = p.waves * 32 * p.qt;
  p.nqt = (int)cdiv(nq, p.wq);
  p.nq_pad = (int64_t)p.nqt * p.wq;
  p.pre_waves = p.dp == 128 ? 4 : p.waves;
  p.nqt_pre = (int)(p.nq_pad / (p.pre_waves * 32 * p.qt));
  // k > 24 (M = 16): twice the lane streams, so that dense neighbourhoods do
  // not overflow a lane's list (10M x 256, k = 200: 2 uncertified queries per
  // 4096 -> 0, and the 4.5 ms fp64 fallback scan with them)
  // pre-pass stride: the pre-pass costs ~nb / stride per query, the main pass
  // admits ~stride * R items above tau per query (list insertions); the best
  // stride grows like sqrt(nb / R): the power of two >= 8 sqrt(nb/1M * 16/R),
  // in [2, 64] (and stride * R >= 4k, above).  Measured at R = 16 (IP, per
  // GPU): 1M x 128 k = 5 -> 8; 10M x 256 k = 5 -> 32 (total 17.0 -> 15.8 ms vs
  // 8); 125K x 128 k = 5, 32768 queries -> 4 (-7 %).  At R = 8 the same rule
  // gives 16, 64 and 8 (1M x 128: stride 16 1.001 ms, 32 1.026 ms)
  {
    const double want = 8.0 * sqrt((double)nb / 1e6 * 16.0 / p.R);
    int st = 2;
    while (st < 64 && st < want) st *= 2;
    if (k > 8)
      while (st < 64 && (int64_t)st * p.R < 4 * (int64_t)k) st *= 2;
    p.tstride = st;
  }
  // workgroups: four rounds of one per CU (two of the 4-wave form run on a CU
  // at a time; the DP = 128 8-wave form, one per CU, takes two rounds, which
  // keeps the chunk count and so the merge's union: 4096 queries -> 64 chunks)
  int target = p.M >= 16 ? 2048 : (p.dp == 128 && p.waves == 8) ? 512 : 1024;
  int64_t nch = target / (p.nqt > 0 ? p.nqt : 1);
  // ... but at least enough chunks (2 lane streams each) that the ~stride * R
  // items above tau spread to <= M per stream: with many query tiles (a
  // corpus shard searched by N x 4096 queries) the workgroup target alone
  // left 16 streams per query and ~1/6 of the queries uncertified at k = 200
  const int64_t min_streams = cdiv((int64_t)p.tstride * p.R, (int64_t)2 * p.M);
  if (nch < min_streams) nch = min_streams;
  if (nch < 1) nch = 1;
  int64_t max_by_u = 2048 / (2 * p.M);
  if (nch > max_by_u) nch = max_by_u;
  int64_t max_by_len = cdiv(nb, 1024);
  if (nch > max_by_len) nch = max_by_len;
  if (nch < 1) nch = 1;
  // buffer descriptors address a chunk with 32-bit offsets: keep chunks < 1 GiB
  const int64_t min_nch = cdiv(nb * (int64_t)p.dp * 2, (int64_t)1 << 30);
  if (nch < min_nch) nch = min_nch;
  p.chunk = (int64_t)align_up((size_t)cdiv(nb, nch), 64);
  p.nch = (int)cdiv(nb, p.chunk);
  p.U = p.nch * 2 * p.M;
  if (p.U > 2048) {  // the merge holds the union in registers (8 entries per thread)
    p.exact_only = true;
    p.cliff = true;
    p.total = 256;
    return p;
  }
  int kp = 2 * k > 32 ? 2 * k : 32;
  if (kp < k + 16) kp = k + 16;
  if (kp > p.U) kp = p.U;
  if (kp > 1024) kp = 1024;
  p.KP = kp;
  if (p.KP < k) {
    p.exact_only = true;
    p.cliff = true;
    p.total = 256;
    return p;
  }
  // pre-pass: every tstride-th 64-item tile, chunks small enough that each
  // query gets >= 8R short lane streams (their maxima are distinct items), but
  // >= 8 visited tiles per workgroup (a small shard searched by many query
  // tiles otherwise launched thousands of 2-tile workgroups)
  {
    const int TI = 64;  // must equal screen_kernel TI
    int64_t tiles = cdiv(nb, TI);
    int64_t want = 4 * p.R;  // 2 lanes per chunk -> 8R streams
    const int64_t min_pre = cdiv(nb * (int64_t)p.dp * 2, (int64_t)1 << 30);
    if (want < min_pre) want = min_pre;
    if (want > 512) want = 512;
    int64_t maxc = cdiv(tiles, (int64_t)p.tstride * 8);
    if (want > maxc) want = maxc;
    if (want < 1) want = 1;
    p.chunk_pre = cdiv(cdiv(tiles, want), p.tstride) * p.tstride * TI;
    p.nch_pre = (int)cdiv(nb, p.chunk_pre);
    if (2 * p.nch_pre < p.R) p.tau = false;
  }
  // Uncertified queries are collected in rounds of FB_SLOTS_MAX (16 K) slots,
  // as many rounds as nq needs (a corpus shard searched by N x 4096 queries
  // leaves more than 4096 of them uncertified at L2; queries beyond a fixed
  // slot budget used to take the block-per-query exact scan: 2.3 s for 574
  // queries over a 2.5M-row shard at world 4).  The tiled fp64 fallback then
  // takes the (rare) queries whose collect buffer overflowed, with storage for
  // candidates at least as good as the merge's k-th; its cap leaves room for
  // 2k + 64 (ties and near-ties), overflow goes to exact_topk.  Each slot holds
  // fb_cap x 16 B of fallback candidates and ccap x 4 B of collect positions
  // (16 KB at k <= 224), so the cap bounds this part of the workspace at 256 MB
  p.fb_slots = (int)(nq < FB_SLOTS_MAX ? nq : FB_SLOTS_MAX);
  p.fb_cap = fallback_cap(k);
  // collect pass: one query tile per wave (128 queries per work item), 4096-row
  // chunks (each chunk's query tiles run back to back on one XCD), storage for
  // the fb_slots uncertified queries that carry an e_k
  p.cwq = 4 * 32;
  p.cch = 4096;
  p.ccap = 2048;
  p.crows = cdiv(p.fb_slots, p.cwq) * p.cwq;
  {
    const int64_t items = (p.crows / p.cwq) * cdiv(nb, (int64_t)p.cch);
    p.cgrid = (int)(items < 512 ? items : 512);  // two 4-wave blocks per CU fill the chip
  }
  FlatWs w;
  p.total = flat_carve(nullptr, p, nq, w);
  return p;
}

}  // namespace nrk

using namespace nrk;

extern "C" int nrk_padded_dim(int32_t d) { return padded_dim(d); }

// The flat search's main-pass screen kernel for a plan.  Inner product: the
// 16x16x32 form where built (NRK_SCREEN16=0: the 32x32x16 kernel, which every
// other form runs; a test hook).
static screen_fn main_pass(const FlatPlan& p, bool l2, bool* s16) {
  *s16 = false;
  // (DP = 128 with 8 waves is planned only for the 16x16x32 form)
  screen_fn fn = p.waves == 8 ? (p.dp == 256 ? pick_screen_dp256_w8(p.M, l2, 0) : nullptr)
                              : pick_screen(p.dp, p.qt, p.M, l2, 0);
  if (!l2 && test_hook("NRK_SCREEN16", 1)) {
    screen_fn f16 = p.waves == 8 ? (p.dp == 256 ? pick_screen16_dp256_w8(p.M) : pick_screen16_dp128_w8(p.qt, p.M))
                                 : (p.dp == 128 ? pick_screen16_dp128(p.qt, p.M) : nullptr);
    if (f16) {
      fn = f16;
      *s16 = true;
    }
  }
  return fn;
}

extern "C" int nrk_knn_flat_main_pass(int64_t nq, int64_t nb, int32_t d, int32_t k, int32_t metric, char* name,
                                      size_t len) {
  NRK_CHECK_ARG(name && len > 0 && nq >= 0 && nb >= 0 && d > 0 && k > 0, "knn_flat_main_pass: bad arguments");
  const bool l2 = metric == NRK_METRIC_L2;
  const FlatPlan p = make_plan(nq, nb, d, k, l2);
  if (p.small) snprintf(name, len, "small_exact (fp64 tile GEMM, no screen)");
  else if (p.exact_only) snprintf(name, len, "exact_topk_kernel (fp64 brute force, no screen)");
  else {
    bool s16 = false;
    (void)main_pass(p, l2, &s16);
    snprintf(name, len, "%s<dp %d, qt %d, M %d, %d waves, %s> (bf16 v_mfma_f32_%s)", s16 ? "screen16_kernel" : "screen_kernel",
             p.dp, p.qt, p.M, p.waves, l2 ? "L2" : "IP", s16 ? "16x16x32" : "32x32x16");
  }
  return NRK_OK;
}

extern "C" int nrk_flat_prepare(const float* xb, int64_t nb, int32_t d, uint16_t* xb_bf16, float* xb_meta,
                                float* stats, void* stream) {
  NRK_CHECK_ARG(d > 0 && nb >= 0, "flat_prepare: bad shape nb=%lld d=%d", (long long)nb, d);
  if (nb == 0) return NRK_OK;
  NRK_CHECK_ARG(xb && xb_bf16 && xb_meta && stats, "flat_prepare: null pointer");
  const int dp = padded_dim(d);
  const int rows_per_block = 4;
  const int64_t blocks = cdiv(nb, rows_per_block) < 8192 ? cdiv(nb, rows_per_block) : 8192;
  hipLaunchKernelGGL(flat_prepare_kernel, dim3((unsigned)blocks), dim3(64 * rows_per_block), 0,
                     (hipStream_t)stream, xb, nb, d, dp, xb_bf16, xb_meta, stats);
  NRK_CHECK_LAUNCH("flat_prepare_kernel");
  return NRK_OK;
}

extern "C" int nrk_knn_flat_workspace(int64_t nq, int64_t nb, int32_t d, int32_t k, size_t* ws_bytes) {
  NRK_CHECK_ARG(ws_bytes && nq >= 0 && nb >= 0 && d > 0 && k > 0, "knn_flat_workspace: bad arguments");
  // (no metric here: the larger of the two plans, which differ where the inner
  // product runs 8-wave workgroups)
  const size_t ip = make_plan(nq, nb, d, k, false).total, l2 = make_plan(nq, nb, d, k, true).total;
  *ws_bytes = ip > l2 ? ip : l2;
  return NRK_OK;
}

extern "C" int nrk_knn_flat(const float* xq, int64_t nq, const float* xb, const uint16_t* xb_bf16,
                            const float* xb_meta, const float* stats, int64_t nb, int32_t d, int32_t k,
                            int32_t metric, float* D, int64_t* I, double* S, int64_t id_offset,
                            int32_t* n_fallback, void* ws, size_t ws_bytes, void* const* stage_events,
                            void* stream) {
  NRK_CHECK_ARG(d > 0 && k > 0 && k <= 1024 && nq >= 0 && nb >= 0, "knn_flat: bad shape nq=%lld nb=%lld d=%d k=%d",
                (long long)nq, (long long)nb, d, k);
  NRK_CHECK_ARG(metric == NRK_METRIC_INNER_PRODUCT || metric == NRK_METRIC_L2, "knn_flat: bad metric %d", metric);
  hipStream_t st = (hipStream_t)stream;
  FlatPlan p = make_plan(nq, nb, d, k, metric == NRK_METRIC_L2);
  // L2: rescore at least the top 128 screened candidates.  The certificate
  // needs the k-th exact score to clear theta (>= the best candidate NOT
  // rescored) by the screening-error bound, which for squared L2 on clustered
  // data often exceeds the gap between the 5th and the 33rd neighbour: 10M x 128
  // k = 5 at KP = 32 left 1125 of 4096 queries to the collect pass (12.9 ms),
  // at KP = 128 4 (10.4 ms); 1M x 128: 74 -> 0, 1.33 -> 1.23 ms.  The workspace
  // does not depend on KP.
  if (metric == NRK_METRIC_L2 && !p.exact_only && p.KP < 128) p.KP = p.U < 128 ? p.U : 128;
  if (ws_bytes < p.total) return fail(NRK_EWORKSPACE, "knn_flat: workspace %zu < %zu bytes", ws_bytes, p.total);
  NRK_CHECK_ARG(ws != nullptr, "knn_flat: null workspace");
  int* fbc = static_cast<int*>(ws);  // the counters: the first region of every plan
  // the screened path zeroes its counters in query_prepare_kernel and publishes
  // them from exact_topk_kernel; the other paths use memsets
  // (the small path zeroes n_fallback in its kernels and uses no counters: no memsets)
  const bool fused_counts = nq > 0 && !p.small && !p.exact_only;
  if (!fused_counts && !p.small) {
    if (hipMemsetAsync(fbc, 0, 16, st) != hipSuccess) return fail(NRK_ELAUNCH, "knn_flat: memset failed");
    if (n_fallback && hipMemsetAsync(n_fallback, 0, 8, st) != hipSuccess)
      return fail(NRK_ELAUNCH, "knn_flat: memset failed");
  }
  if (nq == 0) return NRK_OK;
  NRK_CHECK_ARG(xq && D && I && (xb || nb == 0), "knn_flat: null pointer");
  const int l2 = metric == NRK_METRIC_L2;
  if (p.small) return small_launch(p.sm, xq, nq, xb, nb, d, k, l2, D, I, S, id_offset, ws, st, n_fallback);
  if (p.exact_only) {
    // a shape the screen cannot plan (merge union > 2048, d or k > 256) runs the
    // fp64 brute force for every query: say so through the fallback count
    if (n_fallback && (p.cliff || d > 256 || k > 256) &&
        hipMemsetD32Async(n_fallback, (int)nq, 2, st) != hipSuccess)
      return fail(NRK_ELAUNCH, "knn_flat: memset failed");
    return exact_launch(xq, nq, xb, nb, d, k, l2, nullptr, nullptr, nq, D, I, S, id_offset, st);
  }
  NRK_CHECK_ARG(xb_bf16 && xb_meta && stats, "knn_flat: index not prepared (null bf16/meta/stats)");
  auto mark = [&](int i) {
    if (stage_events) (void)hipEventRecord((hipEvent_t)stage_events[i], st);
  };
  FlatWs w;
  flat_carve(static_cast<char*>(ws), p, nq, w);
  // the merge's uncertified queries (collect pass, in rounds): every one keeps its e_k
  const FbState fb{w.fbl, w.fbc, 0, (int)nq, w.fbt, w.fbi, nullptr, test_hook("NRK_FORCE_FALLBACK", 0)};
  // the tiled fp64 fallback (collect buffer overflow)
  const FbState fbt{w.tfl, w.fbc + 2, p.fb_slots, p.fb_slots, w.tft, w.tfi, w.fbn, 0};
  const float* tau = p.tau ? w.tau : nullptr;

  mark(0);
  int rc = query_prepare_launch(xq, nq, p.nq_pad, d, p.dp, w.qh, w.qmeta, w.fbc, n_fallback, st);
  if (rc != NRK_OK) return rc;
  if (p.tau) {
    screen_fn pf =
        p.pre_waves == 8 ? pick_screen_dp256_w8(p.M, l2 != 0, 1) : pick_screen(p.dp, p.qt, p.M, l2 != 0, 1);
    if (!pf) return fail(NRK_EUNSUPPORTED, "knn_flat: no pre-pass kernel for dp=%d", p.dp);
    hipLaunchKernelGGL(pf, dim3(p.nqt_pre * p.nch_pre), dim3(p.pre_waves * 64), 0, st, w.qh, xb_bf16, xb_meta, nq, nb,
                       p.chunk_pre, p.nch_pre, p.nqt_pre, p.tstride, nullptr, nullptr, w.pre, nullptr, IvfScreen{});
    NRK_CHECK_LAUNCH("screen_kernel (pre-pass)");
    const int nv = 2 * p.nch_pre;
    hipLaunchKernelGGL(tau_select_fn(nv), dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, st, w.pre, nv, p.R, nq, w.tau,
                       nullptr, nullptr);
    NRK_CHECK_LAUNCH("tau_select_kernel");
  }

  bool s16 = false;
  screen_fn fn = main_pass(p, l2 != 0, &s16);
  if (!fn) return fail(NRK_EUNSUPPORTED, "knn_flat: no screen kernel for dp=%d", p.dp);
  const int nblk = p.nqt * p.nch;
  mark(1);
  hipLaunchKernelGGL(fn, dim3(nblk), dim3(p.waves * 64), 0, st, w.qh, xb_bf16, xb_meta, nq, nb, p.chunk, p.nch, p.nqt,
                     1, w.ps, w.pi, w.pt, tau, IvfScreen{});
  NRK_CHECK_LAUNCH("screen_kernel");

  mark(2);
  {
    const int P = pow2ceil(p.U), P2 = pow2ceil(p.KP);
    const size_t ub = (size_t)merge_union_bytes(P, p.KP);
    const size_t smem = ub + (size_t)P2 * 16 + (size_t)d * 4;
    if (smem > 150 * 1024) return fail(NRK_EUNSUPPORTED, "knn_flat: merge needs %zu B LDS", smem);
    hipLaunchKernelGGL(merge_rescore_kernel, dim3((unsigned)nq), dim3(256), smem, st, w.ps, w.pi, w.pt, p.nch, p.M,
                       p.KP, k, p.dp, xq, xb, nb, d, l2, w.qmeta, stats, tau, D, I, S, id_offset, fb);
    NRK_CHECK_LAUNCH("merge_rescore_kernel");
  }

  mark(3);
  {  // collect pass for the uncertified queries (normally none: every launch exits at once)
    screen_fn fc = pick_screen(p.dp, 1, p.M, l2 != 0, 3);
    if (!fc) return fail(NRK_EUNSUPPORTED, "knn_flat: no collect kernel for dp=%d", p.dp);
    IvfScreen isc{w.cwork, w.clo,  w.cseg, w.csp,  1, p.cch, (int)cdiv(nb, (int64_t)p.cch),
                  w.cthr,  w.ccnt, w.cpos, p.ccap, 1};
    const int rounds = (int)cdiv(nq, (int64_t)FB_SLOTS_MAX);
    for (int r = 0; r < rounds; ++r) {  // each round exits at once when it has no queries
      hipLaunchKernelGGL(flat_collect_plan_kernel, dim3(1), dim3(1024), 0, st, fb, nq, nb, p.cwq, p.cch, w.qmeta, stats,
                         p.dp, l2, p.ccap, fb.force >= 2 ? 1 : 0, r, FB_SLOTS_MAX, w.clo, w.cseg, w.cwork, w.csp,
                         w.cthr, w.clbg, w.clbi, w.ccnt, w.clist, w.ccount, w.qh, w.cqi);
      NRK_CHECK_LAUNCH("flat_collect_plan_kernel");
      hipLaunchKernelGGL(fc, dim3((unsigned)p.cgrid), dim3(4 * 64), 0, st, w.cqi, xb_bf16, xb_meta,
                         (int64_t)p.fb_slots, nb, 0, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, isc);
      NRK_CHECK_LAUNCH("screen_kernel (flat collect)");
      rc = collect_rescore_launch(p.fb_slots, w.ccnt, w.cpos, p.ccap, nullptr, xq, xb, d, k, l2, w.clbg, w.clbi, D, I,
                                  S, id_offset, fbt, nq, nb, nullptr, w.clist, w.ccount, st);
      if (rc != NRK_OK) return rc;
    }
  }
  // what the collect pass could not hold; the last launch publishes n_fallback:
  // [0] the queries the certificate did not cover (ccount[1]), [1] the tiled fallback's
  rc = fallback_tail(xq, nq, xb, nb, d, k, l2, fbt, w.fcg, w.fci, p.fb_cap, w.ovl, D, I, S, id_offset, IvfFb{}, st,
                     n_fallback, w.ccount + 1, fbt.count);
  if (rc != NRK_OK) return rc;
  mark(4);
  return NRK_OK;
}

// knn_exact.hip — the fp64 paths of the k-NN searches: every score computed
// exactly in the oracle's operation order (oracle/knn_exact.c), so none of
// them needs a certificate.
//   exact_topk_kernel       block-per-query scan (nrk_knn_exact; small shapes
//                           and shapes the screen cannot plan; the last resort
//                           of both searches' fallback)
//   small_*                 corpus of at most SMALL_NB rows as a tile GEMM
//   fallback_scan / select  chip-wide tiled scan for the slots a search could
//                           not answer from its screened candidates
//   topk_merge_kernel       merge of per-shard results (nrk_topk_merge)
// The searches (knn_flat.hip, ivf_search.hip) reach these through small_launch,
// exact_launch and fallback_tail.
#include "knn_common.h"

namespace nrk {

// ============================================================ exact top-k ==
// Workgroups loop over a query list (fallback) or over all queries (direct
// exact mode).  Block top-k kept in LDS: list [0,k), staged candidates
// [k, k+256), bitonic-merged whenever something was staged.
__global__ __launch_bounds__(256) void exact_topk_kernel(
    const float* __restrict__ xq, int64_t nq, const float* __restrict__ xb, int64_t nb, int d, int k,
    int l2, const int* __restrict__ qlist, const int* __restrict__ qcount, float* __restrict__ D,
    int64_t* __restrict__ I, double* __restrict__ S, int64_t id_offset, IvfFb iv,
    int* __restrict__ cnt_out, const int* __restrict__ cnt_a, const int* __restrict__ cnt_b) {
  // the search's fallback counts (final: written by earlier launches) -> the
  // caller's n_fallback (instead of two copy launches)
  if (cnt_out && blockIdx.x == 0 && threadIdx.x == 0) {
    cnt_out[0] = *cnt_a;
    cnt_out[1] = *cnt_b;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int P = pow2ceil(k + 256);
  double* g = reinterpret_cast<double*>(smem);
  int64_t* id = reinterpret_cast<int64_t*>(g + P);
  float* qs = reinterpret_cast<float*>(id + P);
  __shared__ int s_nst, s_cnt;
  const int tid = threadIdx.x;
  const int64_t nwork = qcount ? (int64_t)*qcount : nq;
  for (int64_t wi = blockIdx.x; wi < nwork; wi += gridDim.x) {
    const int64_t qi = qlist ? (int64_t)qlist[wi] : wi;
    if (!guard_ok((uint64_t)qi < (uint64_t)nq, iv.err, GUARD_FB_QUERY)) continue;  // (block-uniform)
    for (int i = tid; i < P; i += 256) {
      g[i] = -INFINITY;
      id[i] = INT64_MAX;
    }
    for (int i = tid; i < d; i += 256) qs[i] = xq[qi * d + i];
    if (tid == 0) {
      s_nst = 0;
      s_cnt = 0;
    }
    __syncthreads();
    const int nrange = iv.pos2id ? iv.nprobe : 1;
    for (int pr = 0; pr < nrange; ++pr) {
    int64_t lo = 0, hi = nb;
    if (iv.pos2id) {
      const int64_t l = iv.probe[qi * iv.nprobe + pr];
      const bool ok = l >= 0 && guard_ok(l < iv.nlist, iv.err, GUARD_PROBE_LIST);
      lo = ok ? iv.list_off[l] : 0;
      hi = ok ? iv.list_off[l + 1] : 0;
    }
    for (int64_t base = lo; base < hi; base += 256) {
      const int64_t pp = base + tid;  // position (== id for a flat index)
      const int64_t i = pp < hi ? (iv.pos2id ? iv.pos2id[pp] : pp) : nb;
      const int cnt = s_cnt;
      const double tg = g[k - 1];
      const int64_t tidx = id[k - 1];
      if (pp < hi) {
        const double s = exact_score(qs, xb + i * d, d, l2 != 0);
        const double gv = l2 ? -s : s;
        if (cnt < k || better(gv, i, tg, tidx)) {
          const int pos = atomicAdd(&s_nst, 1);
          g[k + pos] = gv;
          id[k + pos] = i;
        }
      }
      __syncthreads();
      const int nst = s_nst;
      if (nst > 0) {
        block_bitonic_sort(g, id, P);
        for (int j = k + tid; j < P; j += 256) {
          g[j] = -INFINITY;
          id[j] = INT64_MAX;
        }
        __syncthreads();
        if (tid == 0) {
          s_cnt = cnt + nst < k ? cnt + nst : k;
          s_nst = 0;
        }
      }
      __syncthreads();
    }
    }
    for (int j = tid; j < k; j += 256) write_result(D, I, S, qi * k + j, id[j] != INT64_MAX, g[j], id[j], l2, id_offset);
    __syncthreads();
  }
}

// ============================================================ small corpus ==
// Exact search over a SMALL corpus (nb <= SMALL_NB: the coarse quantizer's
// centroids, k-means assignment, IndexIVFFlat.add): the (query, item) scores
// are computed EXACTLY in fp64 with the oracle's operation order (sequential d,
// fma) as a 64 x 64 tile GEMM on the VALU — one tile per workgroup, a 4 x 4
// register micro-tile per thread, f32 operands staged d-major through LDS —
// so no certificate is needed.  k = 1 fuses the arg-best into the tile loop
// (a workgroup walks all items for its 64 queries); larger k writes the
// goodness matrix of a query chunk and selects per query with a block bitonic
// sort (P = pow2ceil(nb) <= SMALL_NB entries in LDS).
constexpr int SM_T = 64;          // queries and items per tile
constexpr int SM_DC = 32;         // dimensions staged per LDS step
constexpr int SM_LD = SM_T + 4;   // LDS row stride (floats): conflict-light transposed stores

template <bool L2>
__device__ __forceinline__ void small_tile(const float* __restrict__ xq, int64_t q0, int64_t nq,
                                           const float* __restrict__ xb, int64_t j0, int64_t nb, int d,
                                           float* __restrict__ Qs, float* __restrict__ Xs, double (&acc)[4][4]) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  for (int dc = 0; dc < d; dc += SM_DC) {
    const int w = d - dc < SM_DC ? d - dc : SM_DC;
    __syncthreads();  // previous step's readers are done
#pragma unroll
    for (int u = 0; u < (SM_T * SM_DC) / 256; ++u) {
      const int e = tid + u * 256;
      const int r = e / SM_DC, c = e % SM_DC;  // consecutive threads: consecutive dims of one row
      const int64_t qi = q0 + r, xi = j0 + r;
      Qs[c * SM_LD + r] = (c < w && qi < nq) ? xq[qi * d + dc + c] : 0.f;
      Xs[c * SM_LD + r] = (c < w && xi < nb) ? xb[xi * d + dc + c] : 0.f;
    }
    __syncthreads();
    for (int j = 0; j < w; ++j) {
      const float4 qv = *reinterpret_cast<const float4*>(Qs + j * SM_LD + ty * 4);
      const float4 xv = *reinterpret_cast<const float4*>(Xs + j * SM_LD + tx * 4);
      const double qd[4] = {(double)qv.x, (double)qv.y, (double)qv.z, (double)qv.w};
      const double xd[4] = {(double)xv.x, (double)xv.y, (double)xv.z, (double)xv.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (L2) {
            const double t = qd[r] - xd[c];
            acc[r][c] = fma(t, t, acc[r][c]);
          } else {
            acc[r][c] = fma(qd[r], xd[c], acc[r][c]);
          }
        }
    }
  }
}

// k = 1: grid = query tiles; each workgroup walks every item tile.
template <bool L2>
__global__ __launch_bounds__(256) void small_best_kernel(const float* __restrict__ xq, int64_t nq,
                                                         const float* __restrict__ xb, int64_t nb, int d,
                                                         float* __restrict__ D, int64_t* __restrict__ I,
                                                         double* __restrict__ S, int64_t id_offset,
                                                         int32_t* __restrict__ nfb) {
  __shared__ __attribute__((aligned(16))) float Qs[SM_DC * SM_LD];
  __shared__ __attribute__((aligned(16))) float Xs[SM_DC * SM_LD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  if (nfb && blockIdx.x == 0 && tid < 2) nfb[tid] = 0;  // n_fallback: the exact path answers every query
  const int64_t q0 = (int64_t)blockIdx.x * SM_T;
  double bg[4];
  int64_t bi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    bg[r] = -INFINITY;
    bi[r] = INT64_MAX;
  }
  for (int64_t j0 = 0; j0 < nb; j0 += SM_T) {
    double acc[4][4];
    small_tile<L2>(xq, q0, nq, xb, j0, nb, d, Qs, Xs, acc);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t j = j0 + tx * 4 + c;
      if (j < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double g = L2 ? -acc[r][c] : acc[r][c];
          if (better(g, j, bg[r], bi[r])) {
            bg[r] = g;
            bi[r] = j;
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // arg-best over the 16 lanes sharing these rows
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const double og = __shfl_xor(bg[r], o, 64);
      const int64_t oi = __shfl_xor(bi[r], o, 64);
      if (better(og, oi, bg[r], bi[r])) {
        bg[r] = og;
        bi[r] = oi;
      }
    }
    const int64_t qi = q0 + ty * 4 + r;
    if (tx == 0 && qi < nq) write_result(D, I, S, qi, bi[r] != INT64_MAX, bg[r], bi[r], L2, id_offset);
  }
}

// k > 1, pass 1: goodness G[q - q0][j] for one query chunk; grid = (item tiles, query tiles).
template <bool L2>
__global__ __launch_bounds__(256) void small_scores_kernel(const float* __restrict__ xq, int64_t q0, int64_t nq,
                                                           const float* __restrict__ xb, int64_t nb, int d,
                                                           double* __restrict__ G, int64_t ldg) {
  __shared__ __attribute__((aligned(16))) float Qs[SM_DC * SM_LD];
  __shared__ __attribute__((aligned(16))) float Xs[SM_DC * SM_LD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t j0 = (int64_t)blockIdx.x * SM_T;
  const int64_t qt = q0 + (int64_t)blockIdx.y * SM_T;
  double acc[4][4];
  small_tile<L2>(xq, qt, nq, xb, j0, nb, d, Qs, Xs, acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t qi = qt + ty * 4 + r;
    if (qi >= nq) continue;
    double* row = G + (qi - q0) * ldg + j0 + tx * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (j0 + tx * 4 + c < nb) row[c] = L2 ? -acc[r][c] : acc[r][c];
  }
}

// Few queries (nq < SM_T: the reference's one-profile-at-a-time loop,
// Retrieval.py:28-34): one thread per (query, item) instead of 64 x 64 tiles,
// so nb items spread over nb threads rather than over nb / 64 tile workgroups
// (small_best_kernel spent 188 us on one query over 300 centroids in one
// workgroup).  The arithmetic is small_tile's: fp64 over the dims in order,
// (q - x)^2 or q x fma'd into one accumulator, so the goodness is bit-identical.
template <bool L2>
__global__ __launch_bounds__(256) void small_rows_kernel(const float* __restrict__ xq, int64_t q0, int64_t nc,
                                                         const float* __restrict__ xb, int64_t nb, int d,
                                                         double* __restrict__ G, int64_t ldg) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nc * nb) return;
  const int64_t ql = e / nb, j = e - ql * nb;
  const float* q = xq + (q0 + ql) * d;
  const float* x = xb + j * d;
  double acc = 0.0;
  int c = 0;
  if ((d & 3) == 0) {
    for (; c < d; c += 4) {
      const float4 qv = *reinterpret_cast<const float4*>(q + c);
      const float4 xv = *reinterpret_cast<const float4*>(x + c);
      const double qd[4] = {(double)qv.x, (double)qv.y, (double)qv.z, (double)qv.w};
      const double xd[4] = {(double)xv.x, (double)xv.y, (double)xv.z, (double)xv.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (L2) {
          const double t = qd[u] - xd[u];
          acc = fma(t, t, acc);
        } else {
          acc = fma(qd[u], xd[u], acc);
        }
      }
    }
  }
  for (; c < d; ++c) {
    const double qd = q[c], xd = x[c];
    if (L2) {
      const double t = qd - xd;
      acc = fma(t, t, acc);
    } else {
      acc = fma(qd, xd, acc);
    }
  }
  G[ql * ldg + j] = L2 ? -acc : acc;
}

// k > 1, pass 1 on 32 x 32 tiles (2 x 2 outputs per thread) where 64 x 64 tiles
// give the chip too few workgroups (the coarse quantizer: 4096 queries x 300
// centroids is 320 of them); the same fp64 arithmetic per output.
constexpr int S2_T = 32, S2_LD = S2_T + 2;
template <bool L2>
__global__ __launch_bounds__(256) void small_scores32_kernel(const float* __restrict__ xq, int64_t q0, int64_t nq,
                                                             const float* __restrict__ xb, int64_t nb, int d,
                                                             double* __restrict__ G, int64_t ldg) {
  __shared__ __attribute__((aligned(16))) float Qs[SM_DC * S2_LD];
  __shared__ __attribute__((aligned(16))) float Xs[SM_DC * S2_LD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t j0 = (int64_t)blockIdx.x * S2_T;
  const int64_t qt = q0 + (int64_t)blockIdx.y * S2_T;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int dc = 0; dc < d; dc += SM_DC) {
    const int w = d - dc < SM_DC ? d - dc : SM_DC;
    __syncthreads();  // previous step's readers are done
#pragma unroll
    for (int u = 0; u < (S2_T * SM_DC) / 256; ++u) {
      const int e = tid + u * 256;
      const int r = e / SM_DC, c = e % SM_DC;
      const int64_t qi = qt + r, xi = j0 + r;
      Qs[c * S2_LD + r] = (c < w && qi < nq) ? xq[qi * d + dc + c] : 0.f;
      Xs[c * S2_LD + r] = (c < w && xi < nb) ? xb[xi * d + dc + c] : 0.f;
    }
    __syncthreads();
    for (int j = 0; j < w; ++j) {
      const float2 qv = *reinterpret_cast<const float2*>(Qs + j * S2_LD + ty * 2);
      const float2 xv = *reinterpret_cast<const float2*>(Xs + j * S2_LD + tx * 2);
      const double qd[2] = {(double)qv.x, (double)qv.y};
      const double xd[2] = {(double)xv.x, (double)xv.y};
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          if (L2) {
            const double t = qd[r] - xd[c];
            acc[r][c] = fma(t, t, acc[r][c]);
          } else {
            acc[r][c] = fma(qd[r], xd[c], acc[r][c]);
          }
        }
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int64_t qi = qt + ty * 2 + r;
    if (qi >= nq) continue;
    double* row = G + (qi - q0) * ldg + j0 + tx * 2;
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (j0 + tx * 2 + c < nb) row[c] = L2 ? -acc[r][c] : acc[r][c];
  }
}

// k > 1, pass 2: one workgroup per query of the chunk sorts its nb goodness values.
__global__ __launch_bounds__(256) void small_select_kernel(const double* __restrict__ G, int64_t ldg, int64_t q0,
                                                           int64_t nq, int64_t nb, int k, int l2, int P,
                                                           float* __restrict__ D, int64_t* __restrict__ I,
                                                           double* __restrict__ S, int64_t id_offset,
                                                           int32_t* __restrict__ nfb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* g = reinterpret_cast<double*>(smem);
  int64_t* id = reinterpret_cast<int64_t*>(g + P);
  if (nfb && blockIdx.x == 0 && threadIdx.x < 2) nfb[threadIdx.x] = 0;
  const int64_t qi = q0 + blockIdx.x;
  if (qi >= nq) return;
  const double* row = G + (int64_t)blockIdx.x * ldg;
  for (int i = threadIdx.x; i < P; i += 256) {
    const bool ok = i < nb;
    g[i] = ok ? row[i] : -INFINITY;
    id[i] = ok ? (int64_t)i : INT64_MAX;
  }
  __syncthreads();
  block_bitonic_sort(g, id, P);
  for (int j = threadIdx.x; j < k; j += 256) {
    const bool valid = j < P && id[j] != INT64_MAX;  // (k may exceed the P sorted entries)
    write_result(D, I, S, qi * k + j, valid, valid ? g[j] : 0.0, valid ? id[j] : 0, l2, id_offset);
  }
}

// k <= SW_K and nb <= 64 * VPL (the coarse quantizer: nlist centroids, k =
// nprobe): one wave per query, VPL goodness values per lane in registers, k
// rounds of wave argmax in the bitonic sort's order (goodness descending, id
// ascending).  A block sort per query spends most of its time in barriers.
constexpr int SW_K = 64;
// (value, index) argmax over the wave, every lane receiving the winner: larger
// value first, ties -> lower index (a total order, so any combining tree picks
// the same winner).  DPP row ops and the CDNA4 permlane swaps instead of
// __shfl_xor, which moves each 32-bit half through a ds_bpermute round trip (18
// dependent LDS trips per selection round: 46 us for 4096 queries at k = 32).
__device__ __forceinline__ void am_take(double& v, int& i, double ov, int oi) {
  // bitwise | and & (no short circuit): the compiler otherwise branches on exec
  // masks at every step (two s_cbranch per step, ~39 us for 4096 queries at k = 32)
  const bool t = (ov > v) | ((ov == v) & (oi < i));
  v = t ? ov : v;
  i = t ? oi : i;
}
template <int CTRL>
__device__ __forceinline__ void am_dpp(double& v, int& i) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
  const int oi = __builtin_amdgcn_mov_dpp(i, CTRL, 0xf, 0xf, true);
  am_take(v, i, __hiloint2double(hi, lo), oi);
}
__device__ __forceinline__ void am_swap(double& v, int& i, bool half32) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const auto rl = half32 ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false)
                         : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto rh = half32 ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false)
                         : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const auto ri = half32 ? __builtin_amdgcn_permlane32_swap(i, i, false, false)
                         : __builtin_amdgcn_permlane16_swap(i, i, false, false);
  double a = __hiloint2double((int)rh[0], (int)rl[0]);
  int ia = (int)ri[0];
  am_take(a, ia, __hiloint2double((int)rh[1], (int)rl[1]), (int)ri[1]);
  v = a;
  i = ia;
}
__device__ __forceinline__ void wave_argmax(double& v, int& i) {
  am_dpp<0xB1>(v, i);   // quad_perm [1,0,3,2]
  am_dpp<0x4E>(v, i);   // quad_perm [2,3,0,1]
  am_dpp<0x141>(v, i);  // row_half_mirror
  am_dpp<0x140>(v, i);  // row_mirror
  am_swap(v, i, false); // rows 2k <-> 2k+1
  am_swap(v, i, true);  // halves
}
template <int VPL>
__global__ __launch_bounds__(256) void small_select_wave_kernel(const double* __restrict__ G, int64_t ldg, int64_t q0,
                                                                int64_t nc, int64_t nq, int64_t nb, int k, int l2,
                                                                float* __restrict__ D, int64_t* __restrict__ I,
                                                                double* __restrict__ S, int64_t id_offset,
                                                                int32_t* __restrict__ nfb) {
  const int lane = threadIdx.x & 63;
  if (nfb && blockIdx.x == 0 && threadIdx.x < 2) nfb[threadIdx.x] = 0;
  const int64_t ql = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t qi = q0 + ql;
  if (ql >= nc || qi >= nq) return;
  const double* row = G + ql * ldg;
  double v[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int64_t i = (int64_t)j * 64 + lane;
    v[j] = i < nb ? row[i] : -INFINITY;
  }
  for (int r = 0; r < k; ++r) {
    // the lane's best (an extracted entry reads -inf; it can only win once no
    // real item is left, i.e. r >= nb): first item, then strictly greater, so
    // the lowest index wins ties
    double bv = -INFINITY;
    int bj = VPL;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
      if (((int64_t)j * 64 + lane < nb) & ((bj == VPL) | (v[j] > bv))) {
        bv = v[j];
        bj = j;
      }
    int bi = bj < VPL ? bj * 64 + lane : INT_MAX;
    wave_argmax(bv, bi);
    const bool valid = r < nb && bi != INT_MAX;
    if (valid && lane == (bi & 63)) {
#pragma unroll
      for (int j = 0; j < VPL; ++j)
        if (j == (bi >> 6)) v[j] = -INFINITY;
    }
    if (lane == 0) write_result(D, I, S, qi * k + r, valid, bv, bi, l2, id_offset);
  }
}

// ========================================================= tiled fallback ==
// Chip-wide fp64 scan for the fallback slots: 64-row fp32 tiles staged in LDS
// (row stride d+1, so lane = row reads are bank-conflict free), each wave
// scores its tile against slots w, w+4, ... (the query pointer is wave-uniform)
// with exact_score, and keeps the items at least as good as the slot's
// threshold.  Cost = slots x nb x d fp64 FMA, spread over every CU.

__global__ __launch_bounds__(256) void fallback_scan_kernel(const float* __restrict__ xq,
                                                            const float* __restrict__ xb, int64_t nb, int d,
                                                            int l2, FbState fb, double* __restrict__ cand_g,
                                                            int64_t* __restrict__ cand_i, int cap, IvfFb iv) {
  extern __shared__ float tile[];
  const int c0 = *fb.count;
  const int cnt = c0 < fb.slots ? c0 : fb.slots;
  if (cnt == 0) return;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ds = d + 1;
  const int64_t ntiles = cdiv(nb, (int64_t)FB_TR);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t r0 = t * FB_TR;
    const int rows = nb - r0 < FB_TR ? (int)(nb - r0) : FB_TR;
    __syncthreads();
    if (iv.pos2id) {  // IVF: gather rows by id
      for (int e = threadIdx.x; e < rows * d; e += 256) {
        const int r = e / d;
        tile[r * ds + (e - r * d)] = xb[iv.pos2id[r0 + r] * d + (e - r * d)];
      }
    } else if ((d & 3) == 0) {  // 16 float4 loads in flight per thread (one latency per tile)
      const float4* src = reinterpret_cast<const float4*>(xb + r0 * d);
      const int n4 = (rows * d) >> 2;
      for (int e0 = threadIdx.x; e0 < n4; e0 += 256 * 16) {
        float4 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int e = e0 + u * 256;
          if (e < n4) v[u] = src[e];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int e = e0 + u * 256;
          if (e < n4) {
            const int f = 4 * e, r = f / d;
            float* o = tile + r * ds + (f - r * d);
            o[0] = v[u].x;
            o[1] = v[u].y;
            o[2] = v[u].z;
            o[3] = v[u].w;
          }
        }
      }
    } else {
      for (int e = threadIdx.x; e < rows * d; e += 256) {
        const int r = e / d;
        tile[r * ds + (e - r * d)] = xb[r0 * d + e];
      }
    }
    __syncthreads();
    if (lane >= rows) continue;
    const float* row = tile + lane * ds;
    const int64_t item = iv.pos2id ? iv.pos2id[r0 + lane] : r0 + lane;
    const int mylist = iv.pos2id ? iv.pos2list[r0 + lane] : 0;
    for (int s = wv; s < cnt; s += 4) {
      const int qi = fb.list[s];
      if (iv.nq > 0 && !guard_ok((uint64_t)qi < (uint64_t)iv.nq, iv.err, GUARD_FB_QUERY)) continue;
      if (iv.pos2id) {
        bool member = false;
        for (int pr = 0; pr < iv.nprobe; ++pr) member |= iv.probe[(int64_t)qi * iv.nprobe + pr] == mylist;
        if (!member) continue;
      }
      const double acc = exact_score(xq + (int64_t)qi * d, row, d, l2 != 0);
      const double gv = l2 ? -acc : acc;
      const int64_t ti = fb.thr_i[s];
      if (item == ti || better(gv, item, fb.thr_g[s], ti)) {
        const int pos = atomicAdd(&fb.n[s], 1);
        if (pos < cap) {
          cand_g[(int64_t)s * cap + pos] = gv;
          cand_i[(int64_t)s * cap + pos] = item;
        }
      }
    }
  }
}

// Per slot: sort the collected candidates and write the top k.  Slots whose
// list overflowed (or that have no storage) go to the overflow list, which the
// block-per-query exact kernel finishes.
__global__ __launch_bounds__(256) void fallback_select_kernel(FbState fb, const double* __restrict__ cand_g,
                                                              const int64_t* __restrict__ cand_i, int cap, int k,
                                                              int l2, float* __restrict__ D, int64_t* __restrict__ I,
                                                              double* __restrict__ S, int64_t id_offset,
                                                              int* __restrict__ ov_list, int64_t nq,
                                                              int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* g = reinterpret_cast<double*>(smem);
  int64_t* id = reinterpret_cast<int64_t*>(g + pow2ceil(cap));  // the sort pads n up to a power of two
  const int cnt = *fb.count;
  const int tid = threadIdx.x;
  for (int s = blockIdx.x; s < cnt; s += gridDim.x) {
    const int qi = fb.list[s];
    if (!guard_ok((uint64_t)qi < (uint64_t)nq, err, GUARD_FB_QUERY)) continue;  // (block-uniform)
    const int n = s < fb.slots ? fb.n[s] : cap + 1;
    if (n > cap || n < k) {
      if (tid == 0) ov_list[atomicAdd(&fb.count[1], 1)] = qi;
      continue;
    }
    const int P = pow2ceil(n);
    for (int i = tid; i < P; i += 256) {
      g[i] = i < n ? cand_g[(int64_t)s * cap + i] : -INFINITY;
      id[i] = i < n ? cand_i[(int64_t)s * cap + i] : INT64_MAX;
    }
    __syncthreads();
    block_bitonic_sort(g, id, P);
    for (int j = tid; j < k; j += 256) write_result(D, I, S, (int64_t)qi * k + j, true, g[j], id[j], l2, id_offset);
    __syncthreads();
  }
}

// ============================================================ shard merge ==
__global__ void topk_merge_kernel(const double* __restrict__ Sp, const int64_t* __restrict__ Ip, int nparts,
                                  int64_t nq, int k, int l2, float* __restrict__ D, int64_t* __restrict__ I,
                                  double* __restrict__ S) {
  const int64_t qi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (qi >= nq) return;
  int pos[16];
  for (int p = 0; p < nparts; ++p) pos[p] = 0;
  for (int j = 0; j < k; ++j) {
    int best = -1;
    double bg = 0.0;
    int64_t bi = 0;
    for (int p = 0; p < nparts; ++p) {
      if (pos[p] >= k) continue;
      const int64_t o = ((int64_t)p * nq + qi) * k + pos[p];
      const int64_t ii = Ip[o];
      if (ii < 0) continue;
      const double gv = l2 ? -Sp[o] : Sp[o];
      if (best < 0 || better(gv, ii, bg, bi)) {
        best = p;
        bg = gv;
        bi = ii;
      }
    }
    write_result(D, I, S, qi * k + j, best >= 0, bg, bi, l2, 0);  // (shard ids carry their offsets)
    if (best >= 0) pos[best]++;
  }
}

// ============================================================= launchers ==
SmallPlan make_small_plan(int64_t nq, int64_t nb, int k) {
  SmallPlan p;
  p.P = pow2ceil(nb > 0 ? (int)nb : 1);
  p.ld = align_up((size_t)(nb > 0 ? nb : 1), SM_T);
  const int64_t want = ((int64_t)64 << 20) / (p.ld * 8);  // <= 64 MB of goodness per chunk
  p.chunk = want < SM_T ? SM_T : want / SM_T * SM_T;
  if (p.chunk > (int64_t)align_up((size_t)nq, SM_T)) p.chunk = align_up((size_t)nq, SM_T);
  // (k = 1 with a full query tile: small_best_kernel, no goodness buffer)
  p.ws_bytes = k == 1 && nq >= SM_T ? 256 : align_up((size_t)p.chunk * p.ld * 8, 256);
  return p;
}

template <bool L2>
static int small_launch_metric(const SmallPlan& p, const float* xq, int64_t nq, const float* xb, int64_t nb, int d,
                               int k, float* D, int64_t* I, double* S, int64_t id_offset, void* ws, hipStream_t st,
                               int32_t* nfb) {
  if (k == 1 && nq >= SM_T) {
    const unsigned grid = (unsigned)cdiv(nq, SM_T);
    hipLaunchKernelGGL(small_best_kernel<L2>, dim3(grid), dim3(256), 0, st, xq, nq, xb, nb, d, D, I, S, id_offset, nfb);
    NRK_CHECK_LAUNCH("small_best_kernel");
    return NRK_OK;
  }
  double* G = static_cast<double*>(ws);
  const size_t smem = (size_t)p.P * 16;
  for (int64_t q0 = 0; q0 < nq; q0 += p.chunk) {
    const int64_t nc = nq - q0 < p.chunk ? nq - q0 : p.chunk;
    if (nb > 0 && nc < SM_T) {  // few queries: a thread per (query, item)
      const unsigned grid = (unsigned)cdiv(nc * nb, (int64_t)256);
      hipLaunchKernelGGL(small_rows_kernel<L2>, dim3(grid), dim3(256), 0, st, xq, q0, nc, xb, nb, d, G, p.ld);
      NRK_CHECK_LAUNCH("small_rows_kernel");
    } else if (nb > 0 && cdiv(nb, SM_T) * cdiv(nc, SM_T) < 1024) {  // few tiles: 32 x 32 ones
      const dim3 grid((unsigned)cdiv(nb, S2_T), (unsigned)cdiv(nc, S2_T));
      hipLaunchKernelGGL(small_scores32_kernel<L2>, grid, dim3(256), 0, st, xq, q0, nq, xb, nb, d, G, p.ld);
      NRK_CHECK_LAUNCH("small_scores32_kernel");
    } else if (nb > 0) {
      const dim3 grid((unsigned)cdiv(nb, SM_T), (unsigned)cdiv(nc, SM_T));
      hipLaunchKernelGGL(small_scores_kernel<L2>, grid, dim3(256), 0, st, xq, q0, nq, xb, nb, d, G, p.ld);
      NRK_CHECK_LAUNCH("small_scores_kernel");
    }
    if (k <= SW_K && nb <= 1024) {
      const dim3 g4((unsigned)cdiv(nc, (int64_t)4));
      auto sel = nb <= 256 ? small_select_wave_kernel<4> : nb <= 512 ? small_select_wave_kernel<8>
                                                                     : small_select_wave_kernel<16>;
      hipLaunchKernelGGL(sel, g4, dim3(256), 0, st, G, p.ld, q0, nc, nq, nb, k, (int)L2, D, I, S, id_offset, nfb);
      NRK_CHECK_LAUNCH("small_select_wave_kernel");
    } else {
      hipLaunchKernelGGL(small_select_kernel, dim3((unsigned)nc), dim3(256), smem, st, G, p.ld, q0, nq, nb, k, (int)L2,
                         p.P, D, I, S, id_offset, nfb);
      NRK_CHECK_LAUNCH("small_select_kernel");
    }
  }
  return NRK_OK;
}

int small_launch(const SmallPlan& p, const float* xq, int64_t nq, const float* xb, int64_t nb, int d, int k, int l2,
                 float* D, int64_t* I, double* S, int64_t id_offset, void* ws, hipStream_t st, int32_t* nfb) {
  return l2 ? small_launch_metric<true>(p, xq, nq, xb, nb, d, k, D, I, S, id_offset, ws, st, nfb)
            : small_launch_metric<false>(p, xq, nq, xb, nb, d, k, D, I, S, id_offset, ws, st, nfb);
}

int exact_launch(const float* xq, int64_t nq, const float* xb, int64_t nb, int d, int k, int l2, const int* qlist,
                 const int* qcount, int64_t max_work, float* D, int64_t* I, double* S, int64_t id_offset,
                 hipStream_t st, IvfFb iv, int* cnt_out, const int* cnt_a, const int* cnt_b) {
  const int P = pow2ceil(k + 256);
  const size_t smem = (size_t)P * 16 + (size_t)d * 4;
  if (smem > 160 * 1024) return fail(NRK_EUNSUPPORTED, "exact search: k=%d d=%d needs %zu B of LDS", k, d, smem);
  int grid = (int)(max_work < 2048 ? max_work : 2048);
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(exact_topk_kernel, dim3(grid), dim3(256), smem, st, xq, nq, xb, nb, d, k, l2, qlist, qcount,
                     D, I, S, id_offset, iv, cnt_out, cnt_a, cnt_b);
  NRK_CHECK_LAUNCH("exact_topk_kernel");
  return NRK_OK;
}

int fallback_tail(const float* xq, int64_t nq, const float* xb, int64_t nb, int d, int k, int l2, FbState fb,
                  double* cand_g, int64_t* cand_i, int cap, int* ov_list, float* D, int64_t* I, double* S,
                  int64_t id_offset, IvfFb iv, hipStream_t st, int* cnt_out, const int* cnt_a, const int* cnt_b) {
  if (nb > 0) {
    const int64_t ntiles = cdiv(nb, (int64_t)FB_TR);
    const int grid = (int)(ntiles < 2048 ? ntiles : 2048);
    hipLaunchKernelGGL(fallback_scan_kernel, dim3(grid), dim3(256), (size_t)FB_TR * (d + 1) * 4, st, xq, xb, nb, d,
                       l2, fb, cand_g, cand_i, cap, iv);
    NRK_CHECK_LAUNCH("fallback_scan_kernel");
  }
  hipLaunchKernelGGL(fallback_select_kernel, dim3(256), dim3(256), (size_t)pow2ceil(cap) * 16, st, fb, cand_g, cand_i,
                     cap, k, l2, D, I, S, id_offset, ov_list, nq, iv.err);
  NRK_CHECK_LAUNCH("fallback_select_kernel");
  return exact_launch(xq, nq, xb, nb, d, k, l2, ov_list, fb.count + 1, 256, D, I, S, id_offset, st, iv, cnt_out, cnt_a,
                      cnt_b);
}

}  // namespace nrk

using namespace nrk;

extern "C" int nrk_knn_exact(const float* xq, int64_t nq, const float* xb, int64_t nb, int32_t d, int32_t k,
                             int32_t metric, float* D, int64_t* I, double* S, int64_t id_offset, void* stream) {
  NRK_CHECK_ARG(d > 0 && k > 0 && k <= 1024 && nq >= 0 && nb >= 0, "knn_exact: bad shape nq=%lld nb=%lld d=%d k=%d",
                (long long)nq, (long long)nb, d, k);
  NRK_CHECK_ARG(metric == NRK_METRIC_INNER_PRODUCT || metric == NRK_METRIC_L2, "knn_exact: bad metric %d", metric);
  if (nq == 0) return NRK_OK;
  NRK_CHECK_ARG(xq && D && I && (xb || nb == 0), "knn_exact: null pointer");
  return exact_launch(xq, nq, xb, nb, d, k, metric == NRK_METRIC_L2, nullptr, nullptr, nq, D, I, S, id_offset,
                      (hipStream_t)stream);
}

extern "C" int nrk_topk_merge(const double* S_parts, const int64_t* I_parts, int32_t nparts, int64_t nq, int32_t k,
                              int32_t metric, float* D, int64_t* I, double* S, void* stream) {
  NRK_CHECK_ARG(nparts >= 1 && nparts <= 16 && k > 0 && nq >= 0, "topk_merge: bad arguments nparts=%d k=%d", nparts,
                k);
  NRK_CHECK_ARG(metric == NRK_METRIC_INNER_PRODUCT || metric == NRK_METRIC_L2, "topk_merge: bad metric %d", metric);
  if (nq == 0) return NRK_OK;
  NRK_CHECK_ARG(S_parts && I_parts && D && I, "topk_merge: null pointer");
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, S_parts,
                     I_parts, nparts, nq, k, metric == NRK_METRIC_L2, D, I, S);
  NRK_CHECK_LAUNCH("topk_merge_kernel");
  return NRK_OK;
}

// Multi-output losses (scs_set_outputs): K = nout outputs on one dense A (N x d, panel-blocked).
// The variable is x = vec(X), X d x K column-major; the target Y is N x K column-major.
//
//   Z = A X          multi_ax    (reads A once for all K columns; column-split partials summed
//                                 by the epilogue in a fixed order, as gemv_n)
//   per sample       multi_epilogue (row softmax with the row maximum subtracted | residual of the
//                                 multi-target least squares; R, P, s and the loss partials)
//   G = Aᵀ V         multi_atv   (reads A once; per-chunk column partials, then gemv_t's finalize)
//   w_kl             multi_weight   (one N-vector of the per-sample K x K blocks of Q)
//   placement        multi_place    (a d x d Gram into blocks (k, l) and (l, k) of the d·K system)
//   minibatch        multi_gather_rows (a batch's rows of A and of Y in one launch)
//
// The operands of the two products are repacked K-contiguous first (Xt[j][l], Vt[n][l]): the kernels
// then read the K values of a feature / a sample with wave-uniform addresses (scalar loads for X).
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace scs {

// Xt[j*K + l] = X[j + d*l] for j < d, 0 for d <= j < dpad
__global__ void multi_pack_x_kernel(const double* __restrict__ x, int64_t d, int64_t dpad, int K,
                                    double* __restrict__ Xt) {
  const int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (o >= dpad * K) return;
  const int64_t j = o / K;
  const int l = (int)(o - j * K);
  Xt[o] = (j < d) ? x[j + d * l] : 0.0;
}

hipError_t launch_multi_pack_x(const double* x, int64_t d, int64_t dpad, int K, double* Xt, hipStream_t st) {
  hipLaunchKernelGGL(multi_pack_x_kernel, dim3((unsigned)ceil_div(dpad * K, 256)), dim3(256), 0, st, x, d, dpad, K, Xt);
  return hipGetLastError();
}

// Vt[n*K + l] = V[n + ldv*l] for n < Npad (V's rows N..Npad are zero: the epilogue writes them so)
__global__ void multi_pack_v_kernel(const double* __restrict__ V, int64_t ldv, int64_t Npad, int K,
                                    double* __restrict__ Vt) {
  const int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (o >= Npad * K) return;
  const int64_t n = o / K;
  const int l = (int)(o - n * K);
  Vt[o] = V[n + ldv * l];
}

hipError_t launch_multi_pack_v(const double* V, int64_t ldv, int64_t Npad, int K, double* Vt, hipStream_t st) {
  hipLaunchKernelGGL(multi_pack_v_kernel, dim3((unsigned)ceil_div(Npad * K, 256)), dim3(256), 0, st, V, ldv, Npad, K,
                     Vt);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Z = A X: gemv_n's shape (thread = 2 consecutive samples, 16-B loads along the sample axis, columns
// [c0, c1) whole panels per blockIdx.y) with K accumulator pairs per thread.  Per column the sum runs
// over the split's features in ascending order; part[(split*K + l)*Npad + n].
// ---------------------------------------------------------------------------
constexpr int MX_ROWS = 512;

template <typename TA, int K>
__global__ __launch_bounds__(256) void multi_ax_kernel(const TA* __restrict__ A, int64_t S, int64_t Npad,
                                                       int64_t dpad, const double* __restrict__ Xt, int64_t cps,
                                                       double* __restrict__ part) {
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  if (r >= Npad) return;
  const int64_t c0 = (int64_t)blockIdx.y * cps;
  const int64_t c1 = (c0 + cps < dpad) ? c0 + cps : dpad;
  v2d acc[K];
#pragma unroll
  for (int l = 0; l < K; ++l) acc[l] = (v2d){0.0, 0.0};
  for (int64_t pc = c0; pc < c1; pc += 128) {
    const TA* p = A + tiled_off(S, r, pc);
    const double* xp = Xt + pc * K;
    for (int f = 0; f < 128; f += 8) {
      v2d a[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = ld_pair(p + 16 * (f + i));
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int l = 0; l < K; ++l) acc[l] += a[i] * xp[(f + i) * K + l];
      }
    }
  }
#pragma unroll
  for (int l = 0; l < K; ++l) *(v2d*)(part + ((int64_t)blockIdx.y * K + l) * Npad + r) = acc[l];
}

template <typename TA>
static void multi_ax_dispatch(int K, dim3 grid, hipStream_t st, const TA* A, int64_t S, int64_t Npad, int64_t dpad,
                              const double* Xt, int64_t cps, double* part) {
#define SCS_MAX_CASE(KK)                                                                                        \
  case KK:                                                                                                      \
    hipLaunchKernelGGL((multi_ax_kernel<TA, KK>), grid, dim3(256), 0, st, A, S, Npad, dpad, Xt, cps, part);      \
    break;
  switch (K) {
    SCS_MAX_CASE(1) SCS_MAX_CASE(2) SCS_MAX_CASE(3) SCS_MAX_CASE(4) SCS_MAX_CASE(5) SCS_MAX_CASE(6) SCS_MAX_CASE(7)
    SCS_MAX_CASE(8) SCS_MAX_CASE(9) SCS_MAX_CASE(10) SCS_MAX_CASE(11) SCS_MAX_CASE(12) SCS_MAX_CASE(13)
    SCS_MAX_CASE(14) SCS_MAX_CASE(15) SCS_MAX_CASE(16)
  }
#undef SCS_MAX_CASE
}

hipError_t launch_multi_ax(const void* A, int a32, int64_t S, int64_t Npad, int64_t dpad, int K, const double* Xt,
                           int nsplit, double* part, hipStream_t st) {
  if (K < 1 || K > 16) return hipErrorInvalidValue;
  const int64_t np = dpad / 128;
  const int64_t pps = ceil_div(np, nsplit);   // panels per split
  const int ns = (int)ceil_div(np, pps);
  // unused trailing splits (if any) are zeroed so the epilogue can sum nsplit slices
  if (ns < nsplit) {
    hipError_t e = hipMemsetAsync(part + (int64_t)ns * K * Npad, 0, sizeof(double) * K * Npad * (nsplit - ns), st);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)ceil_div(Npad, MX_ROWS), (unsigned)ns);
  if (a32) multi_ax_dispatch<float>(K, grid, st, (const float*)A, S, Npad, dpad, Xt, pps * 128, part);
  else multi_ax_dispatch<double>(K, grid, st, (const double*)A, S, Npad, dpad, Xt, pps * 128, part);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// G = Aᵀ V: gemv_t_panel_kernel's shape (one workgroup per 4096-row chunk and 128-feature panel, the
// panel's stage blocks streamed in address order; thread (f0, sc) takes features f0 + 32 k and the
// samples 2 sc, 2 sc + 1 of every stage) with K sums per feature.  Per (feature, column) a thread
// adds its two samples of each stage in ascending order, then the 8 lanes of a feature sum in a
// fixed butterfly.  part[(chunk*K + l)*dpad + j]; no atomics.
// ---------------------------------------------------------------------------
constexpr int MT_ROWS = 4096;

int multi_atv_chunks(int64_t Npad) { return (int)ceil_div(Npad, MT_ROWS); }

template <typename TA, int K>
__global__ __launch_bounds__(256) void multi_atv_kernel(const TA* __restrict__ A, int64_t S, int64_t Npad, int64_t d,
                                                        int64_t dpad, const double* __restrict__ Vt,
                                                        double* __restrict__ part) {
  const int64_t r0 = (int64_t)blockIdx.x * MT_ROWS;
  const int ns = (int)(((Npad - r0 < MT_ROWS) ? Npad - r0 : MT_ROWS) / 16);   // Npad % 16 == 0
  const int tid = threadIdx.x, sc = tid & 7, f0 = tid >> 3;
  const TA* blk = A + ((int64_t)blockIdx.y * S + r0 / 16) * (128 * 16) + f0 * 16 + 2 * sc;
  const double* vp = Vt + (r0 + 2 * sc) * K;
  double acc[4][K];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int l = 0; l < K; ++l) acc[k][l] = 0.0;
#pragma unroll 2
  for (int s = 0; s < ns; ++s) {
    const TA* b = blk + (int64_t)s * (128 * 16);
    v2d a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = ld_pair(b + 32 * 16 * k);
    const double* v0 = vp + (int64_t)s * 16 * K;   // samples 2 sc and 2 sc + 1: 2 K contiguous doubles
#pragma unroll
    for (int l = 0; l < K; ++l) {
      const double va = v0[l], vb = v0[K + l];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[k][l] += a[k][0] * va;
        acc[k][l] += a[k][1] * vb;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t j = (int64_t)blockIdx.y * 128 + f0 + 32 * k;
#pragma unroll
    for (int l = 0; l < K; ++l) {
      double t = acc[k][l];
      t += __shfl_xor(t, 1);
      t += __shfl_xor(t, 2);
      t += __shfl_xor(t, 4);
      if (sc == 0 && j < d) part[((int64_t)blockIdx.x * K + l) * dpad + j] = t;
    }
  }
}

template <typename TA>
static void multi_atv_dispatch(int K, dim3 grid, hipStream_t st, const TA* A, int64_t S, int64_t Npad, int64_t d,
                               int64_t dpad, const double* Vt, double* part) {
#define SCS_MTV_CASE(KK)                                                                                        \
  case KK:                                                                                                      \
    hipLaunchKernelGGL((multi_atv_kernel<TA, KK>), grid, dim3(256), 0, st, A, S, Npad, d, dpad, Vt, part);       \
    break;
  switch (K) {
    SCS_MTV_CASE(1) SCS_MTV_CASE(2) SCS_MTV_CASE(3) SCS_MTV_CASE(4) SCS_MTV_CASE(5) SCS_MTV_CASE(6) SCS_MTV_CASE(7)
    SCS_MTV_CASE(8) SCS_MTV_CASE(9) SCS_MTV_CASE(10) SCS_MTV_CASE(11) SCS_MTV_CASE(12) SCS_MTV_CASE(13)
    SCS_MTV_CASE(14) SCS_MTV_CASE(15) SCS_MTV_CASE(16)
  }
#undef SCS_MTV_CASE
}

hipError_t launch_multi_atv(const void* A, int a32, int64_t S, int64_t Npad, int64_t d, int64_t dpad, int K,
                            const double* Vt, double* part, hipStream_t st) {
  if (K < 1 || K > 16) return hipErrorInvalidValue;
  const dim3 grid((unsigned)multi_atv_chunks(Npad), (unsigned)ceil_div(d, 128));
  if (a32) multi_atv_dispatch<float>(K, grid, st, (const float*)A, S, Npad, d, dpad, Vt, part);
  else multi_atv_dispatch<double>(K, grid, st, (const double*)A, S, Npad, d, dpad, Vt, part);
  return hipGetLastError();
}

// out[j + d*l] = Σ_chunk part[(chunk*K + l)*dpad + j] in chunk order (vec(Aᵀ V), column-major d x K)
__global__ __launch_bounds__(128) void multi_atv_finalize_kernel(const double* __restrict__ part, int nchunk, int K,
                                                                 int64_t dpad, int64_t d, double* __restrict__ out) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int l = blockIdx.y;
  if (j >= d) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int c = 0;
  for (; c + 4 <= nchunk; c += 4) {
    s0 += part[((int64_t)c * K + l) * dpad + j];
    s1 += part[((int64_t)(c + 1) * K + l) * dpad + j];
    s2 += part[((int64_t)(c + 2) * K + l) * dpad + j];
    s3 += part[((int64_t)(c + 3) * K + l) * dpad + j];
  }
  for (; c < nchunk; ++c) s0 += part[((int64_t)c * K + l) * dpad + j];
  out[j + d * l] = (s0 + s1) + (s2 + s3);
}

hipError_t launch_multi_atv_finalize(const double* part, int nchunk, int K, int64_t dpad, int64_t d, double* out,
                                     hipStream_t st) {
  hipLaunchKernelGGL(multi_atv_finalize_kernel, dim3((unsigned)ceil_div(d, 128), (unsigned)K), dim3(128), 0, st, part,
                     nchunk, K, dpad, d, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Epilogue over samples (one sample per thread, epilogue_kernel's block structure and value partials).
// zpart: nsplit slices of K columns (stride Npad each).  Outputs, column-major with stride Npad:
//   EPI_Z                     zout = Z
//   EPI_GRAD | EPI_GGN        gout = R  (softmax: c (s_i P_ik - Y_ik); multi LS: c (Z - Y))
//   EPI_HESS | EPI_GGN        hout = P and sout = s_i = Σ_k Y_ik  (softmax only)
//   EPI_VAL                   valpart: Σ_i Σ_k Y_ik log P_ik | Σ_i Σ_k (Z_ik - Y_ik)²
// log P_ik = (Z_ik - max_i) - log Σ_l exp(Z_il - max_i): finite for any finite logits.  Rows
// N..Npad are written as zeros.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void multi_epilogue_kernel(int loss, int flags, int K,
                                                             const double* __restrict__ zpart, int nsplit,
                                                             const double* __restrict__ Y, int64_t N, int64_t Npad,
                                                             double c, double* __restrict__ zout,
                                                             double* __restrict__ gout, double* __restrict__ hout,
                                                             double* __restrict__ sout,
                                                             double* __restrict__ valpart) {
  __shared__ double sh[4];
  double acc = 0.0;
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool wr = (flags & (EPI_GRAD | EPI_GGN)) != 0;
  const bool wp = (flags & (EPI_HESS | EPI_GGN)) != 0 && loss == SCS_LOSS_SOFTMAX_CE;
  if (n < Npad) {
    double z[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      z[l] = 0.0;
      if (l < K)
        for (int s = 0; s < nsplit; ++s) z[l] += zpart[((int64_t)s * K + l) * Npad + n];
    }
    if (flags & EPI_Z) {
#pragma unroll
      for (int l = 0; l < 16; ++l)
        if (l < K) zout[(int64_t)l * Npad + n] = z[l];
    }
    if (n >= N) {
#pragma unroll
      for (int l = 0; l < 16; ++l)
        if (l < K) {
          if (wr) gout[(int64_t)l * Npad + n] = 0.0;
          if (wp) hout[(int64_t)l * Npad + n] = 0.0;
        }
      if (wp) sout[n] = 0.0;
    } else if (!(flags & ~EPI_Z)) {
      // z alone: Y is not read (it may be null)
    } else if (loss == SCS_LOSS_SOFTMAX_CE) {
      double mx = z[0];
#pragma unroll
      for (int l = 1; l < 16; ++l)
        if (l < K) mx = (z[l] > mx) ? z[l] : mx;
      double e[16], se = 0.0, sy = 0.0;
#pragma unroll
      for (int l = 0; l < 16; ++l)
        if (l < K) {
          e[l] = exp(z[l] - mx);
          se += e[l];
          sy += Y[(int64_t)l * Npad + n];
        }
      const double lse = log(se);
#pragma unroll
      for (int l = 0; l < 16; ++l)
        if (l < K) {
          const double y = Y[(int64_t)l * Npad + n];
          const double p = e[l] / se;
          if (flags & EPI_VAL) acc += y * ((z[l] - mx) - lse);
          if (wr) gout[(int64_t)l * Npad + n] = c * (sy * p - y);
          if (wp) hout[(int64_t)l * Npad + n] = p;
        }
      if (wp) sout[n] = sy;
    } else {   // SCS_LOSS_MULTI_LS
#pragma unroll
      for (int l = 0; l < 16; ++l)
        if (l < K) {
          const double res = z[l] - Y[(int64_t)l * Npad + n];
          if (flags & EPI_VAL) acc += res * res;
          if (wr) gout[(int64_t)l * Npad + n] = res * c;
        }
    }
  }
  if (flags & EPI_VAL) {
    const double s = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) valpart[blockIdx.x] = s;
  }
}

hipError_t launch_multi_epilogue(int loss, int flags, int K, const double* zpart, int nsplit, const double* Y,
                                 int64_t N, int64_t Npad, double c, double* z, double* g, double* h, double* s,
                                 double* valpart, hipStream_t st) {
  if (K < 1 || K > 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(multi_epilogue_kernel, dim3((unsigned)ceil_div(Npad, 256)), dim3(256), 0, st, loss, flags, K,
                     zpart, nsplit, Y, N, Npad, c, z, g, h, s, valpart);
  return hipGetLastError();
}

// Q_i[k, l]: softmax c s_i (δ_kl P_ik - P_ik P_il); multi LS c δ_kl.  The one definition: the feature
// branch's weight vectors and the sample-space assembly form the same bits.
__device__ __forceinline__ double multi_q_entry(int loss, const double* __restrict__ P, const double* __restrict__ sv,
                                                int k, int l, int64_t n, int64_t Npad, double c) {
  if (loss == SCS_LOSS_SOFTMAX_CE) {
    const double pk = P[(int64_t)k * Npad + n], pl = P[(int64_t)l * Npad + n];
    return (k == l) ? c * sv[n] * (pk - pk * pl) : c * sv[n] * (-(pk * pl));
  }
  return (k == l) ? c : 0.0;
}

// w_kl,i = Q_i[k, l] (multi LS: called with k = l only).  Rows N..Npad: 0.
__global__ void multi_weight_kernel(int loss, const double* __restrict__ P, const double* __restrict__ sv, int k,
                                    int l, int64_t N, int64_t Npad, double c, double* __restrict__ w) {
  const int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (n >= Npad) return;
  double v = 0.0;
  if (n < N) v = (loss == SCS_LOSS_SOFTMAX_CE) ? multi_q_entry(loss, P, sv, k, l, n, Npad, c) : c;
  w[n] = v;
}

hipError_t launch_multi_weight(int loss, const double* P, const double* s, int k, int l, int64_t N, int64_t Npad,
                               double c, double* w, hipStream_t st) {
  hipLaunchKernelGGL(multi_weight_kernel, dim3((unsigned)ceil_div(Npad, 256)), dim3(256), 0, st, loss, P, s, k, l, N,
                     Npad, c, w);
  return hipGetLastError();
}

// The d x d Gram Gd (its upper triangle, element (i <= j) at Gd[j*ldd + i]) as blocks (k, l) and
// (l, k) of G (leading dimension ldg): both triangles of both blocks (the block is symmetric).
__global__ void multi_place_kernel(const double* __restrict__ Gd, int64_t ldd, int64_t d, int k, int l,
                                   double* __restrict__ G, int64_t ldg) {
  const int64_t j = blockIdx.y;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < d; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = (i <= j) ? Gd[j * ldd + i] : Gd[i * ldd + j];
    G[(l * d + j) * ldg + (k * d + i)] = v;
    if (k != l) G[(k * d + j) * ldg + (l * d + i)] = v;
  }
}

hipError_t launch_multi_place(const double* Gd, int64_t ldd, int64_t d, int k, int l, double* G, int64_t ldg,
                              hipStream_t st) {
  hipLaunchKernelGGL(multi_place_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(d, 256), 8), (unsigned)d), dim3(256),
                     0, st, Gd, ldd, d, k, l, G, ldg);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// ProxGGNSCORE's sample-space branch of a multi-output loss (scs_set_multi_sample, N·K + 1 <= d·K;
// prox-GGN-SCORE.jl:124-127 with J = I_K ⊗ A).  Rows and columns (i, k) = i + N·k, last index n = N·K:
//   M[(i,k),(j,l)] = δ_ij δ_kl + Q_i[k,l] P_l[i,j],   P_l = A diag(h_l) Aᵀ,  h = 1 ./ Hr
//   M[(i,k), n]    = Σ_l Q_i[k,l] u_l[i],              u_l = A (h_l ∘ λ gr_l)
//   M[n, ·] = e_n,  b = [vec(R); 1],  d_l = -(h_l ∘ Aᵀ B_l + (h_l ∘ λ gr_l) B[n])
// M is row-major with row stride ldm = round_up(n + 1, 128) and zero padding (lu.hip).
// ---------------------------------------------------------------------------
// hP[l*dpad + j] = 1 / Hr[j + d*l] (0 for d <= j < dpad: the Gram's weights of block l, padded as the
// single-output hvec is); hg[j + d*l] = h (λ gr) (vec layout: the operand of A X̃ and of the direction)
__global__ void multi_sample_prep_kernel(const double* __restrict__ Hr, const double* __restrict__ gr, double lam,
                                         int64_t d, int64_t dpad, int K, double* __restrict__ hP,
                                         double* __restrict__ hg) {
  const int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (o >= dpad * K) return;
  const int64_t l = o / dpad, j = o - l * dpad;
  double h = 0.0;
  if (j < d) {
    const int64_t f = j + d * l;
    h = 1.0 / Hr[f];   // Hdiag_inv = 1 ./ Hr_diag (prox-GGN-SCORE.jl:64)
    hg[f] = h * (lam * gr[f]);
  }
  hP[o] = h;
}

hipError_t launch_multi_sample_prep(const double* Hr, const double* gr, double lam, int64_t d, int64_t dpad, int K,
                                    double* hP, double* hg, hipStream_t st) {
  hipLaunchKernelGGL(multi_sample_prep_kernel, dim3((unsigned)ceil_div(dpad * K, 256)), dim3(256), 0, st, Hr, gr, lam,
                     d, dpad, K, hP, hg);
  return hipGetLastError();
}

// Column block l of M from P_l (Ps: symmetric, both triangles, leading dimension ldp): one workgroup
// takes MSA_ROWS rows i of P_l and 512 of its columns, reads each element once and writes it into the K
// blocks (k, l).  The K weights Q_i[k,l] of a row are formed once per workgroup (LDS).  Entry = δ + w·p:
// one product, one add (no contraction).  A thread owns two adjacent columns chosen so that the pair
// is 16-byte aligned in M (ldm is even, so the parity of N·l + j decides it for every row); the pairs
// at the two ends of a row of odd offset are single stores.
constexpr int MSA_ROWS = 8;

__global__ __launch_bounds__(256) void multi_sample_assemble_kernel(int loss, int K, int l,
                                                                    const double* __restrict__ Ps, int64_t ldp,
                                                                    const double* __restrict__ P,
                                                                    const double* __restrict__ sv, int64_t N,
                                                                    int64_t Npad, double c, double* __restrict__ Ms,
                                                                    int64_t ldm) {
  __shared__ double w[MSA_ROWS][16];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * MSA_ROWS;
  if (tid < MSA_ROWS * 16) {
    const int r = tid >> 4, k = tid & 15;
    const int64_t i = i0 + r;
    w[r][k] = (i < N && k < K) ? multi_q_entry(loss, P, sv, k, l, i, Npad, c) : 0.0;
  }
  __syncthreads();
  const int64_t cb = N * l;   // first column of block l
  const int64_t j0 = ((int64_t)blockIdx.x * 256 + tid) * 2 - (cb & 1);
  const bool v0 = j0 >= 0 && j0 < N, v1 = j0 + 1 < N;
  if (!v0 && !v1) return;
  double p0[MSA_ROWS], p1[MSA_ROWS];
#pragma unroll
  for (int r = 0; r < MSA_ROWS; ++r) {
    const int64_t i = i0 + r;
    const double* pr = Ps + i * ldp;
    p0[r] = (i < N && v0) ? pr[j0] : 0.0;
    p1[r] = (i < N && v1) ? pr[j0 + 1] : 0.0;
  }
#pragma unroll
  for (int r = 0; r < MSA_ROWS; ++r) {
    const int64_t i = i0 + r;
    if (i >= N) break;
    for (int k = 0; k < K; ++k) {
      const double wk = w[r][k];
      const double e0 = __dadd_rn((k == l && i == j0) ? 1.0 : 0.0, __dmul_rn(wk, p0[r]));
      const double e1 = __dadd_rn((k == l && i == j0 + 1) ? 1.0 : 0.0, __dmul_rn(wk, p1[r]));
      double* o = Ms + (i + N * k) * ldm + cb + j0;
      if (v0 && v1)
        *(v2d*)o = (v2d){e0, e1};
      else if (v0)
        o[0] = e0;
      else
        o[1] = e1;
    }
  }
}

hipError_t launch_multi_sample_assemble(int loss, int K, int l, const double* Ps, int64_t ldp, const double* P,
                                        const double* s, int64_t N, int64_t Npad, double c, double* Ms, int64_t ldm,
                                        hipStream_t st) {
  if (K < 1 || K > 16 || l < 0 || l >= K || N < 1 || (ldm & 1)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)ceil_div(N + 1, 512), (unsigned)ceil_div(N, MSA_ROWS));
  hipLaunchKernelGGL(multi_sample_assemble_kernel, grid, dim3(256), 0, st, loss, K, l, Ps, ldp, P, s, N, Npad, c, Ms,
                     ldm);
  return hipGetLastError();
}

// What the column blocks leave: one workgroup per row r of the padded system.  r < n = N·K: the last
// column Σ_l Q_i[k,l] u_l[i] (l ascending), the zero padding columns, b[r] = R_ik; r = n: e_n and
// b = 1; r > n: zeros.  u and R are N x K with stride Npad.
__global__ __launch_bounds__(128) void multi_sample_tail_kernel(int loss, int K, const double* __restrict__ P,
                                                                const double* __restrict__ sv,
                                                                const double* __restrict__ u,
                                                                const double* __restrict__ R, int64_t N, int64_t Npad,
                                                                double c, double* __restrict__ Ms, int64_t ldm,
                                                                double* __restrict__ b) {
  const int64_t r = blockIdx.x, n = N * K;
  double* row = Ms + r * ldm;
  if (r < n) {
    const int64_t k = r / N, i = r - k * N;
    if (threadIdx.x == 0) {
      double acc = 0.0;
      for (int l = 0; l < K; ++l) acc += multi_q_entry(loss, P, sv, (int)k, l, i, Npad, c) * u[(int64_t)l * Npad + i];
      row[n] = acc;
      b[r] = R[k * Npad + i];
    }
    for (int64_t j = n + 1 + threadIdx.x; j < ldm; j += blockDim.x) row[j] = 0.0;
  } else {
    for (int64_t j = threadIdx.x; j < ldm; j += blockDim.x) row[j] = (r == n && j == n) ? 1.0 : 0.0;
    if (threadIdx.x == 0) b[r] = (r == n) ? 1.0 : 0.0;
  }
}

hipError_t launch_multi_sample_tail(int loss, int K, const double* P, const double* s, const double* u,
                                    const double* R, int64_t N, int64_t Npad, double c, double* Ms, int64_t ldm,
                                    double* b, hipStream_t st) {
  if (K < 1 || K > 16 || N < 1 || ldm < N * K + 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(multi_sample_tail_kernel, dim3((unsigned)ldm), dim3(128), 0, st, loss, K, P, s, u, R, N, Npad, c,
                     Ms, ldm, b);
  return hipGetLastError();
}

// V[i + Npad*l] = B[i + N*l] (rows N..Npad zero): the solution's first N·K entries as the N x K
// operand of Aᵀ V
__global__ void multi_sample_spread_kernel(const double* __restrict__ B, int64_t N, int64_t Npad, int K,
                                           double* __restrict__ V) {
  const int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (o >= Npad * K) return;
  const int64_t l = o / Npad, i = o - l * Npad;
  V[o] = (i < N) ? B[i + N * l] : 0.0;
}

hipError_t launch_multi_sample_spread(const double* B, int64_t N, int64_t Npad, int K, double* V, hipStream_t st) {
  hipLaunchKernelGGL(multi_sample_spread_kernel, dim3((unsigned)ceil_div(Npad * K, 256)), dim3(256), 0, st, B, N, Npad,
                     K, V);
  return hipGetLastError();
}

// d[j + d*l] = -(h_l[j] t[j + d*l] + hg[j + d*l] B[n]), t = vec(Aᵀ V) (the single-output direction's form)
__global__ void multi_sample_direction_kernel(const double* __restrict__ hP, const double* __restrict__ t,
                                              const double* __restrict__ hg, const double* __restrict__ B, int64_t n,
                                              int64_t d, int64_t dpad, int K, double* __restrict__ dir) {
  const int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (f >= d * K) return;
  const int64_t l = f / d, j = f - l * d;
  dir[f] = -(hP[l * dpad + j] * t[f] + hg[f] * B[n]);
}

hipError_t launch_multi_sample_direction(const double* hP, const double* t, const double* hg, const double* B,
                                         int64_t n, int64_t d, int64_t dpad, int K, double* dir, hipStream_t st) {
  hipLaunchKernelGGL(multi_sample_direction_kernel, dim3((unsigned)ceil_div(d * K, 256)), dim3(256), 0, st, hP, t, hg, B,
                     n, d, dpad, K, dir);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Minibatch gather of a multi-output context (scs_set_multi_batches): rows[0..n) of the panel-blocked A
// (S stages, dpad columns) and of Y (N x K, stride ldy) -> the panel-blocked batch Ab (Sb stages, the
// source's element type) and Yb (stride 16 Sb); rows n..16 Sb are zero in both.  One workgroup per
// (16-row output stage, 128-feature panel): thread tid owns batch row t = tid & 15 and the features
// (tid >> 4) + 16 i, reads its source row index once, forms the source block's base once and issues its
// eight loads before its eight stores; a wave's store covers 64 consecutive elements of the output
// block.  The workgroups of panel 0 also write the stage's 16 x K targets.
// ---------------------------------------------------------------------------
template <typename TA>
__global__ __launch_bounds__(256) void multi_gather_rows_kernel(const TA* __restrict__ A, int64_t S,
                                                                const double* __restrict__ Y, int64_t ldy,
                                                                const int64_t* __restrict__ rows, int64_t n,
                                                                int64_t Sb, int K, TA* __restrict__ Ab,
                                                                double* __restrict__ Yb) {
  const int64_t s = blockIdx.x, p = blockIdx.y;
  const int t = threadIdx.x & 15, f0 = threadIdx.x >> 4;
  const int64_t r = s * 16 + t;
  const int64_t src = (r < n) ? rows[r] : -1;
  TA v[8];
  if (src >= 0) {
    const TA* q = A + tiled_off(S, src, 128 * p) + 16 * f0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = q[256 * i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (TA)0;
  }
  TA* o = Ab + ((p * Sb + s) * 128 + f0) * 16 + t;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[256 * i] = v[i];
  if (p == 0)
    for (int l = f0; l < K; l += 16) Yb[(int64_t)l * Sb * 16 + r] = (src >= 0) ? Y[(int64_t)l * ldy + src] : 0.0;
}

// Measured at N = 2^20, d = 2048, K = 8, batches of 2^14 rows: both arms move the source's
// 128-B lines at the rate of a copy.  fp32 storage: this kernel 0.413 ms against 0.440 ms (the K - 1
// launches it saves), the reference arm's round medians within 1.5 %.  fp64: 0.810 against 0.795 ms with
// round medians 12 % apart -- no gain beyond the spread, so the other arm stays the default there.
int multi_gather_default(int a32) { return a32 ? 1 : 0; }

hipError_t launch_multi_gather_rows(const void* A, int a32, int64_t Npad, int64_t dpad, const double* Y, int64_t ldy,
                                    int K, const int64_t* rows, int64_t n, int64_t Npad_b, void* Ab, double* Yb,
                                    hipStream_t st) {
  if (K < 1 || K > 16 || Npad % 16 || Npad_b % 16 || dpad % 128 || n > Npad_b || dpad / 128 > 65535)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(Npad_b / 16), (unsigned)(dpad / 128));
  if (a32)
    hipLaunchKernelGGL(multi_gather_rows_kernel<float>, grid, dim3(256), 0, st, (const float*)A, Npad / 16, Y, ldy,
                       rows, n, Npad_b / 16, K, (float*)Ab, Yb);
  else
    hipLaunchKernelGGL(multi_gather_rows_kernel<double>, grid, dim3(256), 0, st, (const double*)A, Npad / 16, Y, ldy,
                       rows, n, Npad_b / 16, K, (double*)Ab, Yb);
  return hipGetLastError();
}

}  // namespace scs

// Sample-space (length-N) kernels: the two streaming passes over A and the
// per-sample loss epilogue, plus on-device synthetic data.
//
//   z = A*x         gemv_n   (HBM-bound: reads A once, 8·N·m bytes)
//   per-sample      epilogue (sums the z partials in a fixed order, then the
//                    loss value / gradient coefficient / Hessian weight /
//                    GGN (w = s²q, v = s·r) of the selected loss kind)
//   Aᵀ*v            gemv_t   (HBM-bound: reads A once; v staged in LDS)
//
// A is panel-blocked (common.h tiled_off; S = Npad / 16 stages, m_pad % 128 == 0,
// zero rows beyond N and zero columns beyond m).
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace scs {

// ---------------------------------------------------------------------------
// z = A x : 256 threads x 2 rows (16-B loads along the contiguous sample
// axis), columns split over blockIdx.y when there are too few row blocks.
// ---------------------------------------------------------------------------
constexpr int GN_ROWS = 512;

int gemv_n_splits(int64_t Npad, int64_t m) {
  const int64_t rb = ceil_div(Npad, GN_ROWS);
  int64_t s = ceil_div(2048, rb);
  const int64_t smax = ceil_div(m, 128);   // splits are whole panels
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  return (int)s;
}

// thread = 2 consecutive samples (one v2d of a block row); a wave covers 8
// stages, so each load instruction reads 8 full 128-B lines.  Columns [c0, c1)
// are whole panels; x must be zero beyond m (callers pass m_pad-sized x).
// TA (here and below): the stored element type of A, double or float (scs_set_dense_f32); a float
// A is widened in the load (ld_pair), the arithmetic and its order are the fp64 kernel's.
template <typename TA>
__global__ __launch_bounds__(256) void gemv_n_kernel(const TA* __restrict__ A, int64_t S, int64_t Npad,
                                                     int64_t mpad, const double* __restrict__ x, int64_t cps,
                                                     double* __restrict__ part, int64_t ldo) {
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  if (r >= Npad) return;
  const int64_t c0 = (int64_t)blockIdx.y * cps;
  const int64_t c1 = (c0 + cps < mpad) ? c0 + cps : mpad;
  v2d acc0 = {0.0, 0.0}, acc1 = {0.0, 0.0};
  for (int64_t pc = c0; pc < c1; pc += 128) {
    const TA* p = A + tiled_off(S, r, pc);
    const double* xp = x + pc;
#pragma unroll 4
    for (int f = 0; f < 128; f += 8) {
      const v2d a0 = ld_pair(p + 16 * (f + 0));
      const v2d a1 = ld_pair(p + 16 * (f + 1));
      const v2d a2 = ld_pair(p + 16 * (f + 2));
      const v2d a3 = ld_pair(p + 16 * (f + 3));
      const v2d a4 = ld_pair(p + 16 * (f + 4));
      const v2d a5 = ld_pair(p + 16 * (f + 5));
      const v2d a6 = ld_pair(p + 16 * (f + 6));
      const v2d a7 = ld_pair(p + 16 * (f + 7));
      acc0 += a0 * xp[f];
      acc1 += a1 * xp[f + 1];
      acc0 += a2 * xp[f + 2];
      acc1 += a3 * xp[f + 3];
      acc0 += a4 * xp[f + 4];
      acc1 += a5 * xp[f + 5];
      acc0 += a6 * xp[f + 6];
      acc1 += a7 * xp[f + 7];
    }
  }
  *(v2d*)(part + (int64_t)blockIdx.y * ldo + r) = acc0 + acc1;
}

hipError_t launch_gemv_n(const void* A, int a32, int64_t S, int64_t Npad, int64_t mpad, const double* x, int nsplit,
                         double* part, int64_t ldo, hipStream_t st) {
  const int64_t np = mpad / 128;
  const int64_t pps = ceil_div(np, nsplit);   // panels per split
  const int ns = (int)ceil_div(np, pps);
  // unused trailing splits (if any) are zeroed so the epilogue can sum nsplit slices
  if (ns < nsplit) {
    hipError_t e = hipMemsetAsync(part + (int64_t)ns * ldo, 0, sizeof(double) * ldo * (nsplit - ns), st);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)ceil_div(Npad, GN_ROWS), (unsigned)ns);
  if (a32)
    hipLaunchKernelGGL(gemv_n_kernel<float>, grid, dim3(256), 0, st, (const float*)A, S, Npad, mpad, x, pps * 128, part,
                       ldo);
  else
    hipLaunchKernelGGL(gemv_n_kernel<double>, grid, dim3(256), 0, st, (const double*)A, S, Npad, mpad, x, pps * 128,
                       part, ldo);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Loss epilogue  (closed forms; see oracle/scsopt_oracle.py Loss for the
// reference expressions they restate, test/test_algs.jl:9-11)
// ---------------------------------------------------------------------------
// one sample per thread: the z-split partial loads of a sample are independent, so a block's
// loads are all in flight at once (2048 samples per block, 8 sequential per thread, made the
// C5 epilogue latency-bound: 26 us at N = 2^20)
constexpr int EPI_PER_BLOCK = 256;

int epilogue_blocks(int64_t Npad) { return (int)ceil_div(Npad, EPI_PER_BLOCK); }

__global__ __launch_bounds__(256) void epilogue_kernel(int loss, int ggn, int flags, const double* __restrict__ zpart,
                                                       int nsplit, int64_t ldz, const double* __restrict__ y,
                                                       int64_t N, int64_t Npad, double c, double* __restrict__ zout,
                                                       double* __restrict__ gout, double* __restrict__ hout,
                                                       double* __restrict__ wout, double* __restrict__ vout,
                                                       double* __restrict__ valpart) {
  __shared__ double sh[4];
  double acc = 0.0;
  const int64_t base = (int64_t)blockIdx.x * EPI_PER_BLOCK;
  for (int k = 0; k < EPI_PER_BLOCK / 256; ++k) {
    const int64_t n = base + k * 256 + threadIdx.x;
    if (n >= Npad) break;
    double z = 0.0;
    for (int s = 0; s < nsplit; ++s) z += zpart[(int64_t)s * ldz + n];
    if (flags & EPI_Z) zout[n] = z;
    if (n >= N) {
      if (flags & EPI_GRAD) gout[n] = 0.0;
      if (flags & EPI_HESS) hout[n] = 0.0;
      if (flags & EPI_GGN) { wout[n] = 0.0; vout[n] = 0.0; }
      if (flags & EPI_SQR) { gout[n] = 0.0; hout[n] = 0.0; }
      continue;
    }
    const double yn = y[n];
    if (loss == SCS_LOSS_LOGISTIC_MARGIN) {
      const double e = exp(-yn * z);
      if (flags & EPI_VAL) acc += log(1.0 + e);
      if (flags & EPI_GRAD) gout[n] = c * ((-yn * e) / (1.0 + e));
      if (flags & EPI_HESS) hout[n] = c * (yn * yn) * e / ((1.0 + e) * (1.0 + e));
    } else if (loss == SCS_LOSS_LOGISTIC_CE) {
      const double e = exp(-z);
      const double yh = 1.0 / (1.0 + e);
      if (flags & EPI_VAL) acc += yn * log(yh) + (1.0 - yn) * log(1.0 - yh);
      if (flags & (EPI_GRAD | EPI_HESS)) {
        const double s = e / ((1.0 + e) * (1.0 + e));
        const double r = -c * (yn / yh - (1.0 - yn) / (1.0 - yh));
        if (flags & EPI_GRAD) gout[n] = s * r;
        if (flags & EPI_HESS) {
          const double q = c * (yn / (yh * yh) + (1.0 - yn) / ((1.0 - yh) * (1.0 - yh)));
          hout[n] = s * s * q + r * (s * (1.0 - 2.0 * yh));
        }
      }
    } else if (loss == SCS_LOSS_LEAST_SQUARES) {
      const double res = z - yn;
      if (flags & EPI_VAL) acc += res * res;
      if (flags & EPI_GRAD) gout[n] = res * c;
      if (flags & EPI_HESS) hout[n] = c;
    }
    if (flags & EPI_GGN) {
      double s, r, q;
      if (ggn == SCS_GGN_SIGMOID_CE) {
        const double e = exp(-z);
        const double yh = 1.0 / (1.0 + e);
        s = e / ((1.0 + e) * (1.0 + e));
        r = -c * (yn / yh - (1.0 - yn) / (1.0 - yh));
        q = c * (yn / (yh * yh) + (1.0 - yn) / ((1.0 - yh) * (1.0 - yh)));
      } else {  // SCS_GGN_LINEAR_LS
        s = 1.0;
        r = (z - yn) * c;
        q = c;
      }
      if (flags & EPI_SQR) {   // sample-space branch: the factors themselves
        gout[n] = s;
        hout[n] = q;
        wout[n] = r;
      } else {
        wout[n] = s * s * q;
        vout[n] = s * r;
      }
    }
  }
  if (flags & EPI_VAL) {
    const double s = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) valpart[blockIdx.x] = s;
  }
}

hipError_t launch_epilogue(int loss, int ggn, int flags, const double* zpart, int nsplit, int64_t ldz,
                           const double* y, int64_t N, int64_t Npad, double c, double* z, double* g, double* h,
                           double* w, double* v, double* valpart, hipStream_t st) {
  hipLaunchKernelGGL(epilogue_kernel, dim3(epilogue_blocks(Npad)), dim3(256), 0, st, loss, ggn, flags, zpart, nsplit,
                     ldz, y, N, Npad, c, z, g, h, w, v, valpart);
  return hipGetLastError();
}

// SCS_LOSS_SAMPLEWISE: the same outputs from the caller's per-sample numbers (val = l, d1 = dl/dz | r,
// d2 = d²l/dz² | q, s = dŷ/dz) instead of a closed form; epilogue_kernel's block structure (256 samples
// per block, block_sum<256>, one partial per block) and, for the GGN products, its operation order.
// Rows N <= n < Npad are written as zeros whatever the caller's buffers hold there (A's padding rows
// are zero, and 0·NaN would poison Aᵀv and the Gram); the buffers are read for n < N only.
__global__ __launch_bounds__(256) void samplewise_epilogue_kernel(int flags, const double* __restrict__ val,
                                                                  const double* __restrict__ d1,
                                                                  const double* __restrict__ d2,
                                                                  const double* __restrict__ sv, int64_t N,
                                                                  int64_t Npad, double* __restrict__ gout,
                                                                  double* __restrict__ hout,
                                                                  double* __restrict__ wout,
                                                                  double* __restrict__ vout,
                                                                  double* __restrict__ valpart) {
  __shared__ double sh[4];
  double acc = 0.0;
  const int64_t n = (int64_t)blockIdx.x * EPI_PER_BLOCK + threadIdx.x;
  if (n < Npad) {
    if (n >= N) {
      if (flags & EPI_GRAD) gout[n] = 0.0;
      if (flags & EPI_HESS) hout[n] = 0.0;
      if (flags & EPI_GGN) { wout[n] = 0.0; vout[n] = 0.0; }
      if (flags & EPI_SQR) { gout[n] = 0.0; hout[n] = 0.0; }
    } else {
      if (flags & EPI_VAL) acc += val[n];
      if (flags & EPI_GRAD) gout[n] = d1[n];
      if (flags & EPI_HESS) hout[n] = d2[n];
      if (flags & EPI_GGN) {
        const double s = sv[n], r = d1[n], q = d2[n];
        if (flags & EPI_SQR) {   // sample-space branch: the factors themselves
          gout[n] = s;
          hout[n] = q;
          wout[n] = r;
        } else {
          wout[n] = s * s * q;
          vout[n] = s * r;
        }
      }
    }
  }
  if (flags & EPI_VAL) {
    const double s = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) valpart[blockIdx.x] = s;
  }
}

hipError_t launch_samplewise_epilogue(int flags, const double* val, const double* d1, const double* d2,
                                      const double* s, int64_t N, int64_t Npad, double* g, double* h, double* w,
                                      double* v, double* valpart, hipStream_t st) {
  hipLaunchKernelGGL(samplewise_epilogue_kernel, dim3(epilogue_blocks(Npad)), dim3(256), 0, st, flags, val, d1, d2, s,
                     N, Npad, g, h, w, v, valpart);
  return hipGetLastError();
}

__global__ __launch_bounds__(1024) void sum_partials_kernel(const double* __restrict__ part, int n,
                                                            double* __restrict__ out) {
  __shared__ double sh[16];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) acc += part[i];
  const double s = block_sum<1024>(acc, sh);
  if (threadIdx.x == 0) out[0] = s;
}

// At (n-major: At[n*ldt + f] = A[f*lda + n]) for the sample-space Gram A diag(h) Aᵀ; zero padded
template <typename TA>
__global__ void transpose_kernel(const TA* __restrict__ A, int64_t Npad, int64_t N, int64_t m,
                                 double* __restrict__ At, int64_t ldt, int64_t nt) {
  const int64_t S = Npad / 16;
  __shared__ double tile[32][33];
  const int64_t f0 = (int64_t)blockIdx.x * 32, n0 = (int64_t)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int64_t f = f0 + j, n = n0 + tx;
    tile[j][tx] = (f < m && n < N) ? (double)A[tiled_off(S, n, f)] : 0.0;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int64_t n = n0 + j, f = f0 + tx;
    if (n < nt && f < ldt) At[n * ldt + f] = tile[tx][j];
  }
}

hipError_t launch_transpose(const void* A, int a32, int64_t Npad, int64_t N, int64_t m, double* At, int64_t ldt,
                            int64_t nt, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(ldt, 32), (unsigned)ceil_div(nt, 32));
  if (a32)
    hipLaunchKernelGGL(transpose_kernel<float>, grid, dim3(256), 0, st, (const float*)A, Npad, N, m, At, ldt, nt);
  else
    hipLaunchKernelGGL(transpose_kernel<double>, grid, dim3(256), 0, st, (const double*)A, Npad, N, m, At, ldt, nt);
  return hipGetLastError();
}

// Minibatch gather (iterate.jl:141-145, 205-207: the DataLoader batch As, ys of a step!):
// rows[0..n) of the panel-blocked A (Npad rows) -> a panel-blocked batch Ab (Npad_b rows,
// zero padding), y -> yb.  Threads walk the OUTPUT layout, so the writes are coalesced.
// TD: the batch's element type (TA, or double from a float A: the sharded sample-space gather).
template <typename TA, typename TD>
__global__ void gather_rows_kernel(const TA* __restrict__ A, int64_t Npad, const double* __restrict__ y,
                                   const int64_t* __restrict__ rows, int64_t n, int64_t Npad_b, int64_t mpad,
                                   TD* __restrict__ Ab, double* __restrict__ yb) {
  const int64_t S = Npad / 16, Sb = Npad_b / 16;
  const int64_t total = Npad_b * mpad;
  for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = o & 15, f = (o >> 4) & 127, ps = o >> 11;   // ((p*Sb + s)*128 + f)*16 + t
    const int64_t s = ps % Sb, p = ps / Sb;
    const int64_t r = s * 16 + t, j = p * 128 + f;
    const int64_t src = (r < n) ? rows[r] : -1;   // -1: a zero row (rows held by other ranks)
    Ab[o] = (src >= 0) ? (TD)A[tiled_off(S, src, j)] : (TD)0;
    if (j == 0) yb[r] = (src >= 0) ? y[src] : 0.0;
  }
}

hipError_t launch_gather_rows(const void* A, int a32, int64_t Npad, const double* y, const int64_t* rows, int64_t n,
                              int64_t Npad_b, int64_t mpad, void* Ab, int b32, double* yb, hipStream_t st) {
  const int64_t total = Npad_b * mpad;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(total, 256), 65536);
  if (b32 && !a32) return hipErrorInvalidValue;   // a batch is never narrower than its source
  if (a32 && b32)
    hipLaunchKernelGGL((gather_rows_kernel<float, float>), dim3(grid), dim3(256), 0, st, (const float*)A, Npad, y, rows,
                       n, Npad_b, mpad, (float*)Ab, yb);
  else if (a32)
    hipLaunchKernelGGL((gather_rows_kernel<float, double>), dim3(grid), dim3(256), 0, st, (const float*)A, Npad, y,
                       rows, n, Npad_b, mpad, (double*)Ab, yb);
  else
    hipLaunchKernelGGL((gather_rows_kernel<double, double>), dim3(grid), dim3(256), 0, st, (const double*)A, Npad, y,
                       rows, n, Npad_b, mpad, (double*)Ab, yb);
  return hipGetLastError();
}

// panel p of A: column-major buffer C (Npad x 128, ld Npad) <-> the tiled blocks of panel p
// (TC -> TA with to_tiled: a double C into a float A rounds to nearest even, the fp32 storage mode's
// conversion of fp64 input; TA -> TC otherwise: widening)
template <typename TC, typename TA>
__global__ void retile_kernel(TC* __restrict__ C, TA* __restrict__ A, int64_t Npad, int64_t p, int to_tiled) {
  const int64_t S = Npad / 16;
  TA* blk = A + p * S * 128 * 16;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < Npad * 128;
       e += (int64_t)gridDim.x * blockDim.x) {
    // e walks the tiled panel contiguously: e = (s*128 + f)*16 + ks
    const int64_t ks = e & 15, f = (e >> 4) & 127, s = e >> 11;
    const int64_t n = s * 16 + ks;
    if (to_tiled) blk[e] = (TA)C[f * Npad + n];
    else C[f * Npad + n] = (TC)blk[e];
  }
}

hipError_t launch_retile(void* C, int c32, void* A, int a32, int64_t Npad, int64_t p, int to_tiled, hipStream_t st) {
  if (c32 && !a32) return hipErrorInvalidValue;   // an fp32 staging buffer serves an fp32 A only
  if (c32)
    hipLaunchKernelGGL((retile_kernel<float, float>), dim3(1024), dim3(256), 0, st, (float*)C, (float*)A, Npad, p,
                       to_tiled);
  else if (a32)
    hipLaunchKernelGGL((retile_kernel<double, float>), dim3(1024), dim3(256), 0, st, (double*)C, (float*)A, Npad, p,
                       to_tiled);
  else
    hipLaunchKernelGGL((retile_kernel<double, double>), dim3(1024), dim3(256), 0, st, (double*)C, (double*)A, Npad, p,
                       to_tiled);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// A strided DEVICE matrix -> the panel-blocked A (scs_set_data_device): element (n, j) of the source
// at src[n*stride_n + j*stride_m], TS = double | float; TD = the stored type.  One workgroup per
// destination block (panel p, stage s: [128 features][16 samples] of TD, contiguous); every element
// of the block is written exactly once, rows n >= N and features j >= m as zeros, so the block needs
// no memset.  Conversions are plain casts, as in retile_kernel (double -> float rounds to nearest
// even, float -> double is exact).  All offsets are 64-bit.
//
// `vec`: the host found the source base and the leading stride aligned for wide loads; otherwise
// (a view that starts at an odd element, an odd leading stride) every element is loaded on its own.
// Both paths fill the same registers / LDS image, so they store the same bits.
// ---------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));
template <typename T> struct vec16;   // 16 bytes of T
template <> struct vec16<double> { typedef v2d type; };
template <> struct vec16<float> { typedef v4f type; };

// Row-major source (stride_m == 1): the block's source is 16 rows of 128 contiguous features.
//   LDS image   tile[16 samples][DT_PITCH] of TS (the SOURCE type: the cast sits on the way out), the
//               128 features of a sample contiguous, DT_PITCH = 132 elements (a 16-B multiple per row).
//   load side   thread t takes one 16-B vector (ES = 2 doubles | 4 floats) per pass: sample
//               k*RPP + t / LPR, features (t % LPR)*ES ..; LPR = 128 / ES lanes cover a row, so a
//               wave reads 1 KiB of one row (double) or 512 B of two (float).  The ds_write_b128 is
//               served 8 consecutive lanes at a time: 128 contiguous bytes of one row, all 32 banks
//               once, whatever the pitch.
//   store side  wave w of pass k owns 1 KiB of the block: FW = 8 (TD double) | 16 (TD float) features
//               x 16 samples.  Lane l takes feature f0 + l % FW and the ED = 2 | 4 samples
//               (l / FW)*ED ..: ED scalar LDS reads (ds_read_b64 | ds_read_b32, served 32 lanes at a
//               time over 32 slots of the element size), one 16-B global store; the wave's 64 stores
//               tile its 1 KiB.  Read i of lanes 0..31 hits slot ((l/FW)*ED + i)*132 + l % FW + f0:
//               TD double: 2*132 = 8 (mod 32), l/FW = 0..3, l % FW = 0..7  -> 32 different slots;
//               TD float : 4*132 = 16 (mod 32), l/FW = 0..1, l % FW = 0..15 -> 32 different slots;
//               lanes 32..63 likewise.  (The compiler pairs the reads into ds_read2_b32 /
//               ds_read2[st64]_b64; the 8-byte form is served 16 lanes at a time over the 32 four-byte
//               banks, where the same arithmetic gives 16 different even banks.)  Neither side has a
//               bank conflict.
// Blocks are numbered panel-fastest, so the workgroups in flight read whole source rows.
constexpr int DT_PITCH = 132;

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void tile_rows_kernel(const TS* __restrict__ src, int64_t stride_n, int64_t N,
                                                        int64_t m, int64_t S, int64_t np, TD* __restrict__ A,
                                                        int vec) {
  typedef typename vec16<TS>::type VS;
  typedef typename vec16<TD>::type VD;
  constexpr int ES = 16 / sizeof(TS), ED = 16 / sizeof(TD);
  constexpr int LPR = 128 / ES, RPP = 256 / LPR, NLD = 16 / RPP;   // lanes per row, rows per pass, passes
  constexpr int FW = 4 * ED, NST = 128 / (4 * FW);                 // features per wave store, store passes
  __shared__ __attribute__((aligned(16))) TS tile[16 * DT_PITCH];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t total = S * np;
  for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const int64_t s = b / np, p = b - s * np;
    const int64_t n0 = s * 16, j0 = p * 128;
    if (vec) {
      VS r[NLD];
#pragma unroll
      for (int k = 0; k < NLD; ++k) {
        const int64_t n = n0 + k * RPP + t / LPR, j = j0 + (t % LPR) * ES;
        VS v = (VS)(TS)0;
        if (n < N) {
          const TS* q = src + n * stride_n + j;
          if (j + ES <= m) v = *(const VS*)q;
          else {
#pragma unroll
            for (int i = 0; i < ES; ++i)
              if (j + i < m) v[i] = q[i];
          }
        }
        r[k] = v;
      }
#pragma unroll
      for (int k = 0; k < NLD; ++k) *(VS*)&tile[(k * RPP + t / LPR) * DT_PITCH + (t % LPR) * ES] = r[k];
    } else {
      TS r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {   // element k*256 + t of the 16 x 128 source piece, row by row
        const int64_t n = n0 + 2 * k + (t >> 7), j = j0 + (t & 127);
        r[k] = (n < N && j < m) ? src[n * stride_n + j] : (TS)0;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) tile[(2 * k + (t >> 7)) * DT_PITCH + (t & 127)] = r[k];
    }
    __syncthreads();
    TD* blk = A + (p * S + s) * (128 * 16);
#pragma unroll
    for (int k = 0; k < NST; ++k) {
      const int f = (k * 4 + w) * FW + lane % FW, nn = (lane / FW) * ED;
      VD o;
#pragma unroll
      for (int i = 0; i < ED; ++i) o[i] = (TD)tile[(nn + i) * DT_PITCH + f];
      *(VD*)(blk + f * 16 + nn) = o;
    }
    __syncthreads();   // the next block's loads overwrite the image
  }
}

// Column-major source (stride_n == 1): feature j offers the 16 samples of a stage as one contiguous
// piece (128 B of doubles, 64 B of floats), which is the destination's own order; no LDS.  The walk is
// retile_kernel's: thread t of pass k writes the 16-B vector k*256 + t of the block, ED = 2 | 4
// consecutive samples of one feature, from ED consecutive source elements (one 8-, 16- or 32-B load
// when `vec`).  Blocks are numbered stage-fastest: source and destination both advance contiguously.
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void tile_cols_kernel(const TS* __restrict__ src, int64_t stride_m, int64_t N,
                                                        int64_t m, int64_t S, int64_t np, TD* __restrict__ A,
                                                        int vec) {
  typedef typename vec16<TD>::type VD;
  constexpr int ED = 16 / sizeof(TD);
  constexpr int AL = (ED * sizeof(TS) < 16) ? ED * sizeof(TS) : 16;   // what `vec` promises
  typedef TS VS __attribute__((ext_vector_type(ED)));
  const int t = threadIdx.x;
  const int64_t total = S * np;
  for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const int64_t p = b / S, s = b - p * S;
    TD* blk = A + b * (128 * 16);
#pragma unroll
    for (int k = 0; k < 2048 / ED / 256; ++k) {
      const int e = (k * 256 + t) * ED;
      const int64_t n = s * 16 + (e & 15), j = p * 128 + (e >> 4);
      VD o = (VD)(TD)0;
      if (j < m && n < N) {
        const TS* q = src + j * stride_m + n;
        if (vec && n + ED <= N) {
          VS v;
          __builtin_memcpy(&v, __builtin_assume_aligned(q, AL), sizeof(VS));
          o = __builtin_convertvector(v, VD);
        } else {
#pragma unroll
          for (int i = 0; i < ED; ++i)
            if (n + i < N) o[i] = (TD)q[i];
        }
      }
      *(VD*)(blk + e) = o;
    }
  }
}

template <typename TS, typename TD>
static hipError_t launch_tile_device_t(const TS* src, int64_t stride_n, int64_t stride_m, int64_t N, int64_t m,
                                       int64_t Npad, int64_t mpad, TD* A, hipStream_t st) {
  const int64_t S = Npad / 16, np = mpad / 128;
  const unsigned grid = (unsigned)std::min<int64_t>(S * np, 0x7fffffff);
  const uintptr_t base = (uintptr_t)src;
  if (stride_m == 1 && (stride_n != 1 || N <= 1)) {
    const int vec = base % 16 == 0 && (stride_n * (int64_t)sizeof(TS)) % 16 == 0;
    hipLaunchKernelGGL((tile_rows_kernel<TS, TD>), dim3(grid), dim3(256), 0, st, src, stride_n, N, m, S, np, A, vec);
  } else {
    constexpr int64_t ED = 16 / sizeof(TD);
    constexpr int64_t AL = (ED * sizeof(TS) < 16) ? ED * sizeof(TS) : 16;
    const int vec = base % AL == 0 && (stride_m * (int64_t)sizeof(TS)) % AL == 0;
    hipLaunchKernelGGL((tile_cols_kernel<TS, TD>), dim3(grid), dim3(256), 0, st, src, stride_m, N, m, S, np, A, vec);
  }
  return hipGetLastError();
}

// src: N x m device matrix, s32: float elements; one of the strides is 1 (the caller checked them
// and the pointer); A: Npad x mpad panel-blocked, a32: float elements
hipError_t launch_tile_device(const void* src, int s32, int64_t stride_n, int64_t stride_m, int64_t N, int64_t m,
                              int64_t Npad, int64_t mpad, void* A, int a32, hipStream_t st) {
  if (stride_n != 1 && stride_m != 1) return hipErrorInvalidValue;
  if (s32 && a32)
    return launch_tile_device_t((const float*)src, stride_n, stride_m, N, m, Npad, mpad, (float*)A, st);
  if (s32) return launch_tile_device_t((const float*)src, stride_n, stride_m, N, m, Npad, mpad, (double*)A, st);
  if (a32) return launch_tile_device_t((const double*)src, stride_n, stride_m, N, m, Npad, mpad, (float*)A, st);
  return launch_tile_device_t((const double*)src, stride_n, stride_m, N, m, Npad, mpad, (double*)A, st);
}

__global__ void ls_pair_kernel(const double* __restrict__ z0, const double* __restrict__ zd, double alpha,
                               int64_t Npad, double* __restrict__ out) {
  for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < Npad; n += (int64_t)gridDim.x * blockDim.x) {
    out[n] = z0[n];
    out[Npad + n] = alpha * zd[n];
  }
}

hipError_t launch_ls_pair(const double* z0, const double* zd, double alpha, int64_t Npad, double* out,
                          hipStream_t st) {
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(Npad, 256), 4096);
  hipLaunchKernelGGL(ls_pair_kernel, dim3(grid), dim3(256), 0, st, z0, zd, alpha, Npad, out);
  return hipGetLastError();
}

// an empty one-wave kernel: a dispatch whose completion timestamp follows everything before it on the
// stream, including work another library (RCCL) made the stream wait for -- the timers' end marker
__global__ void marker_kernel() {}

hipError_t launch_marker(hipStream_t st) {
  hipLaunchKernelGGL(marker_kernel, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

hipError_t launch_sum_partials(const double* part, int n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(1024), 0, st, part, n, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Aᵀ v : block = (4096-row chunk, 64 columns); v chunk staged in LDS, each
// wave owns 16 columns, 4 at a time; lanes stride the contiguous samples.
// ---------------------------------------------------------------------------
constexpr int GT_ROWS = 4096;

int gemv_t_chunks(int64_t Npad) { return (int)ceil_div(Npad, GT_ROWS); }

template <typename TA>
__global__ __launch_bounds__(256) void gemv_t_kernel(const TA* __restrict__ A, int64_t S, int64_t Npad,
                                                     int64_t m, const double* __restrict__ v,
                                                     double* __restrict__ part, int64_t ldp) {
  __shared__ v2d vs[GT_ROWS / 2];
  const int64_t r0 = (int64_t)blockIdx.x * GT_ROWS;
  const int64_t nr = (Npad - r0 < GT_ROWS) ? Npad - r0 : GT_ROWS;
  const int nh = (int)(nr / 2);
  for (int i = threadIdx.x; i < nh; i += 256) vs[i] = *(const v2d*)(v + r0 + 2 * i);
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t jbase = (int64_t)blockIdx.y * 64 + wid * 16;
  for (int cc = 0; cc < 16; cc += 4) {
    const int64_t j = jbase + cc;
    if (j >= m) break;
    v2d acc[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    // columns j..j+3 share a panel (j % 4 == 0): rows of one stage are 16 contiguous samples
    const TA* p0 = A + tiled_off(S, r0, j);
    for (int i = lane; i < nh; i += 64) {
      const v2d vv = vs[i];
      const TA* pi = p0 + (int64_t)(i >> 3) * (128 * 16) + 2 * (i & 7);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (j + q < m) acc[q] += ld_pair(pi + 16 * q) * vv;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double s = wave_sum(acc[q][0] + acc[q][1]);
      if (lane == 0 && j + q < m) part[(int64_t)blockIdx.x * ldp + j + q] = s;
    }
  }
}

// Aᵀ v by panels (r05): one workgroup per (4096-row chunk, 128-feature panel) streams the panel's
// stage blocks (128 features x 16 samples, 16 KiB contiguous) in address order, 4 KiB per sweep: thread
// (f0, sc) takes features f0 + 32 k, samples 2 sc, 2 sc + 1 of every stage, then the 8 lanes of a
// feature sum in a fixed butterfly.  The column-group kernel above reads each block as 2 x 4 x 4
// scattered 512-B pieces (C2: 1.37 ms per pass, 4.8 TB/s).  SCS_GEMV_T=0: the column-group kernel.
template <typename TA>
__global__ __launch_bounds__(256) void gemv_t_panel_kernel(const TA* __restrict__ A, int64_t S, int64_t Npad,
                                                           int64_t m, const double* __restrict__ v,
                                                           double* __restrict__ part, int64_t ldp) {
  const int64_t r0 = (int64_t)blockIdx.x * GT_ROWS;
  const int ns = (int)(((Npad - r0 < GT_ROWS) ? Npad - r0 : GT_ROWS) / 16);   // Npad % 16 == 0
  const int tid = threadIdx.x, sc = tid & 7, f0 = tid >> 3;
  const TA* blk = A + ((int64_t)blockIdx.y * S + r0 / 16) * (128 * 16) + f0 * 16 + 2 * sc;
  const double* vp = v + r0 + 2 * sc;
  v2d acc[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
#pragma unroll 4
  for (int s = 0; s < ns; ++s) {
    const v2d vv = *(const v2d*)(vp + 16 * s);
    const TA* b = blk + (int64_t)s * (128 * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += ld_pair(b + 32 * 16 * k) * vv;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double t = acc[k][0] + acc[k][1];
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 4);
    const int64_t j = (int64_t)blockIdx.y * 128 + f0 + 32 * k;
    if (sc == 0 && j < m) part[(int64_t)blockIdx.x * ldp + j] = t;
  }
}

static bool gemv_t_panel() {   // read per launch (A/B)
  const char* e = getenv("SCS_GEMV_T");
  return !(e && e[0] == '0');
}

hipError_t launch_gemv_t(const void* A, int a32, int64_t S, int64_t Npad, int64_t m, int64_t mpad, const double* v,
                         double* part, hipStream_t st) {
  if (gemv_t_panel()) {
    const dim3 grid((unsigned)gemv_t_chunks(Npad), (unsigned)ceil_div(m, 128));
    if (a32)
      hipLaunchKernelGGL(gemv_t_panel_kernel<float>, grid, dim3(256), 0, st, (const float*)A, S, Npad, m, v, part, mpad);
    else
      hipLaunchKernelGGL(gemv_t_panel_kernel<double>, grid, dim3(256), 0, st, (const double*)A, S, Npad, m, v, part,
                         mpad);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)gemv_t_chunks(Npad), (unsigned)ceil_div(m, 64));
  if (a32)
    hipLaunchKernelGGL(gemv_t_kernel<float>, grid, dim3(256), 0, st, (const float*)A, S, Npad, m, v, part, mpad);
  else
    hipLaunchKernelGGL(gemv_t_kernel<double>, grid, dim3(256), 0, st, (const double*)A, S, Npad, m, v, part, mpad);
  return hipGetLastError();
}

// out[j] = Σ_c part[c][j]: two columns per thread (16-B loads), four interleaved accumulators
// combined in a fixed order, so 4 loads per thread are in flight (one accumulator chain made the
// 64-chunk C5 finalize latency-bound: 27 us for 33.5 MB)
__global__ __launch_bounds__(128) void gemv_t_finalize_kernel(const double* __restrict__ part, int nchunk,
                                                              int64_t ldp, int64_t m, double* __restrict__ out) {
  const int64_t j = 2 * (blockIdx.x * (int64_t)blockDim.x + threadIdx.x);
  if (j >= m) return;
  v2d s0 = {0.0, 0.0}, s1 = {0.0, 0.0}, s2 = {0.0, 0.0}, s3 = {0.0, 0.0};
  int c = 0;
  for (; c + 4 <= nchunk; c += 4) {
    s0 += *(const v2d*)(part + (int64_t)c * ldp + j);
    s1 += *(const v2d*)(part + (int64_t)(c + 1) * ldp + j);
    s2 += *(const v2d*)(part + (int64_t)(c + 2) * ldp + j);
    s3 += *(const v2d*)(part + (int64_t)(c + 3) * ldp + j);
  }
  for (; c < nchunk; ++c) s0 += *(const v2d*)(part + (int64_t)c * ldp + j);
  const v2d s = (s0 + s1) + (s2 + s3);
  out[j] = s[0];
  if (j + 1 < m) out[j + 1] = s[1];
}

hipError_t launch_gemv_t_finalize(const double* part, int nchunk, int64_t mpad, int64_t m, double* out,
                                  hipStream_t st) {
  // ldp = mpad (even, >= m + 1 when m is odd): the pair loads stay inside each partial row
  hipLaunchKernelGGL(gemv_t_finalize_kernel, dim3((unsigned)ceil_div(ceil_div(m, 2), 128)), dim3(128), 0, st, part,
                     nchunk, mpad, m, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Synthetic data: counter-based RNG (splitmix64 finaliser over (seed, index)),
// so every element is a pure function of its global index -> row shards are
// generated in place and agree with any other sharding.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t smix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double uni(uint64_t seed, uint64_t idx) {
  const uint64_t h = smix(smix(seed) ^ idx);
  return ((double)(h >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ double gauss(uint64_t seed, uint64_t idx) {
  const double u1 = uni(seed, 2 * idx), u2 = uni(seed, 2 * idx + 1);
  return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// grid.y = m_pad columns; columns >= m (and rows >= N) are zero; TA = float stores the fp64 value
// rounded to nearest even
template <typename TA>
__global__ void gen_A_kernel(TA* __restrict__ A, int64_t Npad, int64_t N, int64_t m, int64_t row0,
                             uint64_t seed, double scale) {
  const int64_t j = blockIdx.y;
  const int64_t S = Npad / 16;
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < Npad; n += (int64_t)gridDim.x * blockDim.x) {
    double v = 0.0;
    if (n < N && j < m) v = scale * gauss(seed, (uint64_t)(row0 + n) * (uint64_t)m + (uint64_t)j);
    A[tiled_off(S, n, j)] = (TA)v;
  }
}

hipError_t launch_gen_A(void* A, int a32, int64_t Npad, int64_t N, int64_t m, int64_t mpad, int64_t row0,
                        uint64_t seed, double scale, hipStream_t st) {
  int64_t gx = ceil_div(Npad, 256);
  if (gx > 64) gx = 64;
  const dim3 grid((unsigned)gx, (unsigned)mpad);
  if (a32) hipLaunchKernelGGL(gen_A_kernel<float>, grid, dim3(256), 0, st, (float*)A, Npad, N, m, row0, seed, scale);
  else hipLaunchKernelGGL(gen_A_kernel<double>, grid, dim3(256), 0, st, (double*)A, Npad, N, m, row0, seed, scale);
  return hipGetLastError();
}

__global__ void gen_xtrue_kernel(double* __restrict__ x, int64_t m, uint64_t seed, double density) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= m) return;
  x[j] = (uni(seed + 1, j) < density) ? gauss(seed + 2, j) : 0.0;
}

hipError_t launch_gen_xtrue(double* x, int64_t m, uint64_t seed, double density, hipStream_t st) {
  hipLaunchKernelGGL(gen_xtrue_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st, x, m, seed, density);
  return hipGetLastError();
}

__global__ void gen_y_kernel(int kind, const double* __restrict__ z, double* __restrict__ y, int64_t N, int64_t row0,
                             uint64_t seed) {
  const int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (n >= N) return;
  const uint64_t gi = (uint64_t)(row0 + n);
  const double p = 1.0 / (1.0 + exp(-z[n]));
  if (kind == 1) y[n] = (uni(seed + 3, gi) < p) ? 1.0 : 0.0;
  else if (kind == 2) y[n] = (uni(seed + 3, gi) < p) ? 1.0 : -1.0;
  else y[n] = z[n] + 0.1 * gauss(seed + 4, gi);
}

hipError_t launch_gen_y(int kind, const double* z, double* y, int64_t N, int64_t row0, uint64_t seed,
                        hipStream_t st) {
  hipLaunchKernelGGL(gen_y_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, st, kind, z, y, N, row0, seed);
  return hipGetLastError();
}

// out[k][n] = A(n, cols[k]) for n < N (column-major N x ncols): selected columns of the
// panel-blocked A back in the host layout (bench.py's sampled Gram / Aᵀv check)
template <typename TA>
__global__ void get_columns_kernel(const TA* __restrict__ A, int64_t S, const int64_t* __restrict__ cols,
                                   int64_t N, double* __restrict__ out) {
  const int64_t k = blockIdx.y, j = cols[k];
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x)
    out[k * N + n] = (double)A[tiled_off(S, n, j)];
}

hipError_t launch_get_columns(const void* A, int a32, int64_t S, const int64_t* cols, int64_t ncols, int64_t N,
                              double* out, hipStream_t st) {
  if (ncols <= 0 || N <= 0) return hipSuccess;
  const dim3 grid(256, (unsigned)ncols);
  if (a32) hipLaunchKernelGGL(get_columns_kernel<float>, grid, dim3(256), 0, st, (const float*)A, S, cols, N, out);
  else hipLaunchKernelGGL(get_columns_kernel<double>, grid, dim3(256), 0, st, (const double*)A, S, cols, N, out);
  return hipGetLastError();
}

// out[k] = G[ij[k].y * ld + ij[k].x]
__global__ void gather_entries_kernel(const double* __restrict__ G, int64_t ld, const int2* __restrict__ ij, int n,
                                      double* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = G[(int64_t)ij[k].y * ld + ij[k].x];
}

hipError_t launch_gather_entries(const double* G, int64_t ld, const int2* ij, int n, double* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(gather_entries_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, G, ld, ij, n, out);
  return hipGetLastError();
}

}  // namespace scs

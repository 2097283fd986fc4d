// Multi-output losses on a sparse A (scs_set_sparse_outputs): the two products with K right-hand
// sides in one pass over A's nonzeros.
//
//   Z = A X       on the blocked CSR copy (rows = samples, gathered operand = Xt, d x KP packed)
//   vec(Aᵀ V)     on the blocked CSC copy (rows = features, gathered operand = Vt, Npad x KP packed)
//
// Layout: the LDS-blocked copy of sparse.hip (build_blocked: ptr, 16-bit local indices, values,
// segments padded to whole slots) cut at a finer shift, so that the KP-contiguous slice of the packed
// operand fills the LDS the single-vector kernel fills with one column: the sub-block width is
// W = min(2^spmv_blk_shift(ncols), 16384 / KP) indices, KP = K rounded up to a power of two, and the
// staged slice (W + 1 zero row) x KP doubles (128 KiB + KP·8 B at most).  The operand is packed
// KP-contiguous with zero columns beyond K (multi_spmm_pack_kernel), so a slice is one contiguous
// range of it.  KP consecutive sub-blocks form a group -- the 16384-index block of the single-vector
// layout -- and the kernel writes one partial per (group, column): out[(g·K + l)·ldo + r].  The
// partial counts are the single-vector layout's.
//
// Kernel: a workgroup owns (ROWS consecutive rows, one group), ROWS = 1024 or 256 threads; lane = one
// row with KP register accumulators.  (The 256-row form is the batch-shaped geometry of DESIGN §2l: four
// times the workgroups on a view of few rows, four times the staged elements per thread; the LDS layout
// and every (row, column) sum are the 1024-row form's, so both write the same bits.)  Per sub-block of the group: the slice's loads from the packed operand (in parts of
// 8 or 4 per thread, a part's loads all in flight), barrier, the LDS stores, barrier, then each lane
// streams its row's slots of that sub-block (one slot's loads in flight ahead of the compute; the
// row's slot range and first slot of the NEXT sub-block are requested before the staging / under the
// compute, so no iteration starts with two dependent round trips) and adds value·slice[index][l]
// into accumulator l.  The padding index of the copy (spmv_pad_index() = 16384) is clamped to W, the
// zero row, so padding needs no compare and never meets an operand value.  A slice row's 16-byte
// chunks are stored swizzled by the row index (in the kernel): 64 lanes gathering one chunk index of
// 64 scattered rows would otherwise meet on 32 / KP of the 16 four-bank groups.
//
// Sum order per (row, column): within a group the row's entries in ascending index (sub-blocks in
// order, slots in order, the 4 / 8 entries of a slot left to right), one accumulator, one
// multiply-add each, starting from +0.0; the groups are then summed in group order by
// multi_epilogue_kernel (A X) / in multi_atv_finalize_kernel's four-chain order (Aᵀ V).  No atomics:
// the result does not depend on scheduling.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace scs {

constexpr int MSP_THREADS = 1024;        // = rows per workgroup (the wide form: full data, held-out sets)
constexpr int MSP_NARROW = 256;          // ... of the narrow form (sparse batch views only, SpBlkT::narrow)
constexpr int MSP_LDS_IDX = 1 << 14;     // W·KP: the slice without its zero row
constexpr int MSP_PADIDX = 1 << 14;      // build_blocked's padding index (spmv_pad_index())

typedef unsigned long long msp_v2u64 __attribute__((ext_vector_type(2)));
typedef float msp_v4f __attribute__((ext_vector_type(4)));

template <typename VT, int SLOT>
struct MspSlot {
  uint64_t id[SLOT / 4];   // SLOT 16-bit local indices
  VT v[SLOT];              // as stored: fp32 values are widened at the multiply
};

__device__ __forceinline__ void msp_load(MspSlot<double, 4>& w, const uint16_t* __restrict__ lidx,
                                         const double* __restrict__ val, int64_t slot) {
  w.id[0] = *(const uint64_t*)(lidx + 4 * slot);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const v2d a = *(const v2d*)(val + 4 * slot + 2 * k);
    w.v[2 * k] = a[0];
    w.v[2 * k + 1] = a[1];
  }
}
__device__ __forceinline__ void msp_load(MspSlot<float, 8>& w, const uint16_t* __restrict__ lidx,
                                         const float* __restrict__ val, int64_t slot) {
  const msp_v2u64 t = *(const msp_v2u64*)(lidx + 8 * slot);
  w.id[0] = t[0];
  w.id[1] = t[1];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const msp_v4f a = *(const msp_v4f*)(val + 8 * slot + 4 * k);
#pragma unroll
    for (int q = 0; q < 4; ++q) w.v[4 * k + q] = a[q];
  }
}

// the body of both forms: ROWS = the workgroup's threads = its rows
template <typename VT, int SLOT, int KP, int ROWS>
__device__ __forceinline__ void multi_spmm_blk_body(const int64_t* __restrict__ ptr, const uint16_t* __restrict__ lidx,
                                                    const VT* __restrict__ val, const double* __restrict__ Xt, int K,
                                                    /* Xt: ncols x KP, zero beyond column K */
                                                    int64_t nrows, int64_t ncols, int shift, int nsub,
                                                    double* __restrict__ out, int64_t ldo) {
  constexpr int SH = SLOT == 4 ? 2 : 3;
  constexpr int LK = KP == 2 ? 1 : KP == 4 ? 2 : KP == 8 ? 3 : 4;
  static_assert((1 << LK) == KP, "KP is 2, 4, 8 or 16");
  static_assert(ROWS == MSP_THREADS || ROWS == MSP_NARROW, "1024 or 256 rows per workgroup");
  // the slice is staged in NR rounds of NH parts of PER elements per thread (registers: 16 accumulators
  // beside a part); the narrow form keeps NH and PER and takes four rounds (a rolled loop: unrolled, the
  // 4·NH·PER bounds masks of a sub-block do not fit the scalar registers)
  constexpr int NR = MSP_THREADS / ROWS;
  constexpr int NH = KP == 16 ? 4 : 2;
  constexpr int PER = MSP_LDS_IDX / MSP_THREADS / NH;   // staged elements per thread and part
  constexpr int CH = KP / 2;   // 16-byte chunks of a slice row
  __shared__ __attribute__((aligned(256))) double xs[MSP_LDS_IDX + KP];
  const int W = 1 << shift;              // W·KP <= MSP_LDS_IDX (launch_multi_spmm checks)
  const int nslice = W << LK;            // the slice; its zero row follows
  const int g = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * ROWS + threadIdx.x;
  const bool live = r < nrows;
  double acc[KP];
#pragma unroll
  for (int l = 0; l < KP; ++l) acc[l] = 0.0;
  const int sb0 = g * KP, sb1 = min(sb0 + KP, nsub);
  // my row's slots of the first sub-block [q0, q1) and the first of them
  int64_t q0 = 0, q1 = 0;
  if (live) {
    const int64_t* pb = ptr + (int64_t)sb0 * nrows + r;
    q0 = pb[0] >> SH;
    q1 = pb[1] >> SH;
  }
  // (16 accumulators beside three 8-entry slots do not fit 128 registers: that variant loads a
  // sub-block's first slot after the staging instead of under the previous sub-block's compute)
  constexpr bool PF = !(KP == 16 && SLOT == 8);
  MspSlot<VT, SLOT> fst = {};
  if (PF && q0 < q1) msp_load(fst, lidx, val, q0);
#pragma unroll 1
  for (int sb = sb0; sb < sb1; ++sb) {
    const int64_t p0 = q0, p1 = q1;
    q0 = q1 = 0;
    if (live && sb + 1 < sb1) {   // the next sub-block's range: in flight under the staging
      const int64_t* pb = ptr + (int64_t)(sb + 1) * nrows + r;
      q0 = pb[0] >> SH;
      q1 = pb[1] >> SH;
    }
    const int64_t c0 = (int64_t)sb << shift;
    const int nval = (int)min((int64_t)W, ncols - c0) << LK;   // the slice's entries inside the operand
    const double* src = Xt + (c0 << LK);
    // stage the slice in NH parts: a part's loads of a thread all in flight before its LDS stores
    double t[PER];
#pragma unroll 1
    for (int rd = 0; rd < NR; ++rd) {
      const int i0 = threadIdx.x + rd * (NH * PER * ROWS);
#pragma unroll
      for (int h = 0; h < NH; ++h) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          const int i = i0 + (h * PER + k) * ROWS;
          t[k] = (i < nval) ? src[i] : 0.0;
        }
        if (h == 0 && rd == 0) __syncthreads();   // the previous sub-block's gathers are done
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          const int i = i0 + (h * PER + k) * ROWS;
          if (i < nslice) xs[i ^ (((i >> 5) & (CH - 1)) << 1)] = t[k];   // the row's chunks swizzled (below)
        }
      }
    }
    if (threadIdx.x < KP) xs[nslice + threadIdx.x] = 0.0;
    __syncthreads();
    MspSlot<VT, SLOT> nxt = fst;
    if (!PF && p0 < p1) msp_load(nxt, lidx, val, p0);
    if (PF && q0 < q1) msp_load(fst, lidx, val, q0);   // the next sub-block's first slot, under this one's compute
#pragma unroll 1
    for (int64_t p = p0; p < p1; ++p) {
      const MspSlot<VT, SLOT> w = nxt;
      if (p + 1 < p1) msp_load(nxt, lidx, val, p + 1);
#pragma unroll
      for (int e = 0; e < SLOT; ++e) {
        const uint32_t j = min((uint32_t)((w.id[e / 4] >> (16 * (e & 3))) & 0xFFFF), (uint32_t)W);
        // Row j holds its chunk c at position c ^ ((j >> (5 - LK)) & (CH - 1)): a wave reads one chunk
        // index of 64 scattered rows per instruction, and unswizzled rows of KP·8 B put those 64
        // addresses on 16 / CH bank groups of the 16 (a 32-way conflict at KP = 16).
        const uint32_t b2 = (j << (LK + 3)) ^ (((j >> (5 - LK)) & (CH - 1)) << 4);   // bytes
        const double a = (double)w.v[e];
#pragma unroll
        for (int l = 0; l < KP; l += 2) {
          const v2d x2 = *(const v2d*)((const char*)xs + (b2 ^ (uint32_t)(l << 3)));
          acc[l] += a * x2[0];
          acc[l + 1] += a * x2[1];
        }
        // at most 16 gathered doubles in flight: without the fence the scheduler hoists a whole slot's
        // LDS reads (SLOT·KP doubles) above the multiply-adds and the kernel spills at KP >= 8
        if ((e + 1) % (KP >= 16 ? 1 : 16 / KP) == 0) __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  if (live) {
#pragma unroll
    for (int l = 0; l < KP; ++l)
      if (l < K) out[((int64_t)g * K + l) * ldo + r] = acc[l];
  }
}

// the 1024-row form (its name and launch bounds as before the body took ROWS) and the 256-row form
template <typename VT, int SLOT, int KP>
__global__ __launch_bounds__(MSP_THREADS) void multi_spmm_blk_kernel(const int64_t* __restrict__ ptr,
                                                                     const uint16_t* __restrict__ lidx,
                                                                     const VT* __restrict__ val,
                                                                     const double* __restrict__ Xt, int K,
                                                                     int64_t nrows, int64_t ncols, int shift,
                                                                     int nsub, double* __restrict__ out,
                                                                     int64_t ldo) {
  multi_spmm_blk_body<VT, SLOT, KP, MSP_THREADS>(ptr, lidx, val, Xt, K, nrows, ncols, shift, nsub, out, ldo);
}

template <typename VT, int SLOT, int KP>
__global__ __launch_bounds__(MSP_NARROW) void multi_spmm_blk256_kernel(const int64_t* __restrict__ ptr,
                                                                       const uint16_t* __restrict__ lidx,
                                                                       const VT* __restrict__ val,
                                                                       const double* __restrict__ Xt, int K,
                                                                       int64_t nrows, int64_t ncols, int shift,
                                                                       int nsub, double* __restrict__ out,
                                                                       int64_t ldo) {
  multi_spmm_blk_body<VT, SLOT, KP, MSP_NARROW>(ptr, lidx, val, Xt, K, nrows, ncols, shift, nsub, out, ldo);
}

// The packed operand of the kernel above: dst[j*KP + l] = src[j + ld*l] for j < nvalid and l < K, else 0
// (j < ntotal).  x = vec(X): ld = nvalid = d, ntotal = d_pad; an N x K operand V: ld = nvalid = ntotal = N_pad.
__global__ void multi_spmm_pack_kernel(const double* __restrict__ src, int64_t ld, int64_t nvalid, int64_t ntotal,
                                       int K, int lk, double* __restrict__ dst) {
  const int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (o >= (ntotal << lk)) return;
  const int64_t j = o >> lk;
  const int l = (int)(o & ((1 << lk) - 1));
  dst[o] = (j < nvalid && l < K) ? src[j + ld * l] : 0.0;
}

static int msp_kp(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }

int multi_spmm_shift(int64_t ncols, int K) {
  int lk = 1;
  while ((1 << lk) < msp_kp(K)) ++lk;
  return std::min(spmv_blk_shift(ncols), 14 - lk);
}

int multi_spmm_group(int K) { return msp_kp(K); }

// The fallback rule (its one place).  Measured at N = 2^20, d = 2^16, 655 nonzeros per row
// (profiles/multi_sparse/): for K >= 3 and both storage types the one-pass kernel's whole
// range lies below the range of K single-vector launches; at K = 2 it does not (3.9 against 2.3 ms
// fp64, 2.2 against 1.5 ms fp32: the restaging of a 2-column slice costs what a second pass costs).
int multi_spmm_default(int K, int f32) {
  (void)f32;
  return K >= 3;
}

// The narrow form on sparse batch views (its one place).  The rule of §2i / §2k: a form is the default for
// a (KP, storage) only where its whole range over alternated rounds lies below the other's.  Measured on
// 2^14-row views of N = 2^20, d = 2^16, 655 nonzeros per row (profiles/multi_sparse_batches/),
// a step's four products: KP = 8 fp64 0.435 (0.428 .. 0.459) against 0.697 (0.686 .. 0.713) ms, fp32 0.373
// (0.367 .. 0.381) against 0.440 (0.432 .. 0.460); KP = 16 fp64 0.819 (0.813 .. 0.830) against 0.912
// (0.906 .. 0.924), fp32 0.859 (0.852 .. 0.873) against 0.974 (0.963 .. 0.978).  KP = 2 and 4 were not
// measured and keep 1024 rows (SCS_MULTI_SPARSE_NARROW=1 selects the narrow form there).
int multi_spmm_narrow_default(int K, int f32) {
  (void)f32;
  return msp_kp(K) >= 8;
}

const char* multi_spmm_kernel_name(int f32, int K, int narrow) {
  static const char* const names[2][2][4] = {
      {{"multi_spmm_blk_kernel<double, 4, 2>", "multi_spmm_blk_kernel<double, 4, 4>",
        "multi_spmm_blk_kernel<double, 4, 8>", "multi_spmm_blk_kernel<double, 4, 16>"},
       {"multi_spmm_blk_kernel<float, 8, 2>", "multi_spmm_blk_kernel<float, 8, 4>",
        "multi_spmm_blk_kernel<float, 8, 8>", "multi_spmm_blk_kernel<float, 8, 16>"}},
      {{"multi_spmm_blk256_kernel<double, 4, 2>", "multi_spmm_blk256_kernel<double, 4, 4>",
        "multi_spmm_blk256_kernel<double, 4, 8>", "multi_spmm_blk256_kernel<double, 4, 16>"},
       {"multi_spmm_blk256_kernel<float, 8, 2>", "multi_spmm_blk256_kernel<float, 8, 4>",
        "multi_spmm_blk256_kernel<float, 8, 8>", "multi_spmm_blk256_kernel<float, 8, 16>"}}};
  const int kp = msp_kp(K);
  return names[narrow ? 1 : 0][f32 ? 1 : 0][kp == 2 ? 0 : kp == 4 ? 1 : kp == 8 ? 2 : 3];
}

template <typename VT, int SLOT, bool NARROW>
static void msp_dispatch(int kp, dim3 grid, hipStream_t st, const int64_t* ptr, const uint16_t* lidx, const VT* val,
                         const double* Xt, int K, int64_t nrows, int64_t ncols, int shift, int nsub, double* out,
                         int64_t ldo) {
#define SCS_MSP_CASE(KP)                                                                                             \
  case KP:                                                                                                           \
    if (NARROW)                                                                                                      \
      hipLaunchKernelGGL((multi_spmm_blk256_kernel<VT, SLOT, KP>), grid, dim3(MSP_NARROW), 0, st, ptr, lidx, val, Xt, \
                         K, nrows, ncols, shift, nsub, out, ldo);                                                    \
    else                                                                                                             \
      hipLaunchKernelGGL((multi_spmm_blk_kernel<VT, SLOT, KP>), grid, dim3(MSP_THREADS), 0, st, ptr, lidx, val, Xt,   \
                         K, nrows, ncols, shift, nsub, out, ldo);                                                    \
    break;
  switch (kp) { SCS_MSP_CASE(2) SCS_MSP_CASE(4) SCS_MSP_CASE(8) SCS_MSP_CASE(16) }
#undef SCS_MSP_CASE
}

hipError_t launch_multi_spmm_pack(const double* src, int64_t ld, int64_t nvalid, int64_t ntotal, int K, double* dst,
                                  hipStream_t st) {
  if (K < 2 || K > 16) return hipErrorInvalidValue;
  if (ntotal <= 0) return hipSuccess;
  int lk = 1;
  while ((1 << lk) < msp_kp(K)) ++lk;
  hipLaunchKernelGGL(multi_spmm_pack_kernel, dim3((unsigned)ceil_div(ntotal << lk, 256)), dim3(256), 0, st, src, ld,
                     nvalid, ntotal, K, lk, dst);
  return hipGetLastError();
}

hipError_t launch_multi_spmm(const int64_t* ptr, const uint16_t* lidx, const void* val, int f32, const double* Xt,
                             int K, int64_t nrows, int64_t ncols, int shift, double* out, int64_t ldo,
                             hipStream_t st, int narrow) {
  if (K < 2 || K > 16) return hipErrorInvalidValue;
  if (nrows <= 0 || ncols <= 0) return hipSuccess;   // no rows, or nothing to gather from
  const int kp = msp_kp(K);
  if (shift < 0 || ((int64_t)kp << shift) > MSP_LDS_IDX || spmv_pad_index() != MSP_PADIDX) return hipErrorInvalidValue;
  const int nsub = (int)ceil_div(ncols, (int64_t)1 << shift);
  const dim3 grid((unsigned)ceil_div(nrows, narrow ? MSP_NARROW : MSP_THREADS), (unsigned)ceil_div(nsub, kp));
  if (f32 && narrow)
    msp_dispatch<float, 8, true>(kp, grid, st, ptr, lidx, (const float*)val, Xt, K, nrows, ncols, shift, nsub, out,
                                       ldo);
  else if (f32)
    msp_dispatch<float, 8, false>(kp, grid, st, ptr, lidx, (const float*)val, Xt, K, nrows, ncols, shift, nsub, out,
                                        ldo);
  else if (narrow)
    msp_dispatch<double, 4, true>(kp, grid, st, ptr, lidx, (const double*)val, Xt, K, nrows, ncols, shift, nsub,
                                        out, ldo);
  else
    msp_dispatch<double, 4, false>(kp, grid, st, ptr, lidx, (const double*)val, Xt, K, nrows, ncols, shift, nsub,
                                         out, ldo);
  return hipGetLastError();
}

}  // namespace scs

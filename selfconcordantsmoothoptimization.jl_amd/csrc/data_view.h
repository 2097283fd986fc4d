// The N-dependent state of a context -- the data rows, their N-space workspace, the GGN sample-space
// caches and, for a sparse A, its copies -- declared once.  scs_ctx derives from ViewData (the view in
// place); a minibatch, the gathered rows of the sharded GGN branch, the GGN callback's Jacobian and the
// held-out set are NViews exchanged with it for the duration of a call (swap_view), the As, ys handed
// to step! (iterate.jl:205-207).  Pure C++ (no HIP calls), so tests/test_data_view_host.py compiles it
// with the host sanitizers and checks the exchange and the buffer walk without a GPU.
#pragma once
#include <stdint.h>

#include <initializer_list>
#include <utility>

namespace scs {

#ifdef __HIP_PLATFORM_AMD__
using SampleTile = int2;   // the Gram launch list's element (gram_launch_gen)
#else
struct SampleTile {        // its layout, for a host-only build
  int x, y;
};
#endif

// an LDS-blocked copy of a sparse A (sparse.hip)
struct SpBlkT {
  int shift = 0, nblk = 0;
  // blocks per partial: 1 in the single-vector layout; the K-column layout of a multi-output context
  // (scs_set_sparse_outputs, multi_sparse.hip) cuts each 16384-index block into kp sub-blocks and the
  // products still write one partial per group of kp
  int kp = 1;
  // the K-column product's workgroup form on this copy: 0 1024 rows per workgroup, 1 256 (set where a
  // sparse batch view is built, scs_set_multi_sparse_batches; the full data and held-out sets keep 0)
  int narrow = 0;
  int64_t nnz = 0;   // entries of the copy
  int64_t* ptr = nullptr;
  uint16_t* lidx = nullptr;
  void* val = nullptr;
};

// the scratch of a GGN sample-space step on N samples: P, the (N+1)² system and its vectors.  A dense
// view owns one (ViewSample::ss); the sparse branch keeps one per size (scs_ctx::ssys, keyed by N),
// shared by the full data or every batch view of that size
struct SampleSys {
  int64_t N = -1, NpS = 0;
  int64_t n1pad = 0;   // row stride of Ms: round_up(N + 1, 128) (lu.hip)
  double *Ps = nullptr, *Ms = nullptr, *bS = nullptr, *uN = nullptr, *hvec = nullptr, *hg = nullptr;
};

// ---- the parts of a view: what is exchanged together --------------------------------------------
struct ViewRows {
  bool sparse = false;   // a batch view is dense (Matrix(As'), iterate.jl:207) unless it carries the copies
  double* A = nullptr;
  int a32 = 0;   // A holds float elements (scs_set_dense_f32): half the doubles allocated, widened on load
  double* y = nullptr;
  int64_t N = 0, Npad = 0;
  int64_t nstage = 0;   // Npad / 16: stages of the panel-blocked A (common.h tiled_off)
  int64_t Nglob = 0;
};

struct ViewWork {   // the N-space workspace (alloc_nspace)
  int nsplit = 1, nval = 1, nchunk = 1;
  double *zpart = nullptr, *z = nullptr, *gN = nullptr, *hN = nullptr, *wN = nullptr, *vN = nullptr,
         *valpart = nullptr, *tpart = nullptr;
};

struct ViewSample {   // GGN sample-space branch (N + 1 <= m): Aᵀ copy, its Gram's launch list, the system
  double* At = nullptr;
  SampleTile* stiles = nullptr;
  int nstiles = 0;
  SampleSys ss;
};

struct ViewProd {   // a sparse A's entry count and the LDS-blocked copies the products use (sparse.hip)
  int64_t nnz = 0;
  SpBlkT bcsr, bcsc;
};

// the plain CSR (rows) and sgram, the Gram-blocked copy of the CSC (columns cut into
// 2^sparse_gram_shift()-wide blocks of rows, unpadded) that the sparse sample-space branch walks
// (scs_set_sparse_sample; built on first use for the full data, a batch view brings its own)
struct ViewCsr {
  int64_t* rowptr = nullptr;
  int* colidx = nullptr;
  void* val = nullptr;
  SpBlkT sgram;
};

struct ViewData : ViewRows, ViewWork, ViewSample, ViewProd, ViewCsr {
  int sp_f32 = 0;   // the sparse values are float
};

// What a view exchanges beyond the rows, the workspace and the sample space, which every view
// exchanges.  The mask stays with the view object (it is not swapped).
enum : unsigned {
  VP_ROWCOPY = 1,    // nnz, bcsr
  VP_COLCOPY = 2,    // bcsc
  VP_CSR = 4,        // rowptr, colidx, val
  VP_SGRAM = 8,      // sgram
  VP_VALTYPE = 16,   // sp_f32
  VIEW_DENSE = 0,
  // a sparse batch view (scs_set_sparse_batches): the two blocked copies scs_set_sparse would build from
  // A[rows_b, :]; sp_f32 stays the data's
  VIEW_SPARSE = VP_ROWCOPY | VP_COLCOPY,
  // ... which also serves ProxGGNSCORE's sample-space branch (scs_set_sparse_sample): the batch's plain
  // CSR and the Gram-blocked copy of its CSC.  The (n+1)² system scratch is not the view's.
  VIEW_SPARSE_SAMPLE = VIEW_SPARSE | VP_CSR | VP_SGRAM,
  // the held-out set: f's fields only.  A sparse set brings its CSR, the row copy and its value type;
  // the data's bcsc and sgram stay in place
  VIEW_TEST = VP_ROWCOPY | VP_CSR | VP_VALTYPE,
};

struct NView : ViewData {
  unsigned parts = VIEW_DENSE;
};

template <class Part>
inline void swap_part(ViewData& a, ViewData& b) {
  std::swap(static_cast<Part&>(a), static_cast<Part&>(b));
}

// exchange the fields of a and b that a view carrying `parts` brings
inline void swap_view_data(ViewData& a, ViewData& b, unsigned parts) {
  swap_part<ViewRows>(a, b);
  swap_part<ViewWork>(a, b);
  swap_part<ViewSample>(a, b);
  if (parts & VP_ROWCOPY) {
    std::swap(a.nnz, b.nnz);
    std::swap(a.bcsr, b.bcsr);
  }
  if (parts & VP_COLCOPY) std::swap(a.bcsc, b.bcsc);
  if (parts & VP_CSR) {
    std::swap(a.rowptr, b.rowptr);
    std::swap(a.colidx, b.colidx);
    std::swap(a.val, b.val);
  }
  if (parts & VP_SGRAM) std::swap(a.sgram, b.sgram);
  if (parts & VP_VALTYPE) std::swap(a.sp_f32, b.sp_f32);
}

// ---- the device buffers of a view: f(pointer field), once per buffer -----------------------------
enum : unsigned {
  VB_A = 1,
  VB_Y = 2,
  VB_WORK = 4,
  VB_SAMPLE = 8,
  VB_PROD = 16,
  VB_CSR = 32,
  VB_ALL = 63,
  // what scs_batch_info counts as a sparse view's bytes
  VB_SPARSE_VIEW = VB_Y | VB_WORK | VB_PROD | VB_CSR,
};

template <class Blk, class F>
inline void blk_buffers(Blk& B, F&& f) {
  f(B.ptr);
  f(B.lidx);
  f(B.val);
}

template <class Sys, class F>
inline void sys_buffers(Sys& S, F&& f) {
  for (auto* p : {&S.Ps, &S.Ms, &S.bS, &S.uN, &S.hvec, &S.hg}) f(*p);
}

template <class View, class F>
inline void view_buffers(View& v, unsigned groups, F&& f) {
  if (groups & VB_A) f(v.A);
  if (groups & VB_Y) f(v.y);
  if (groups & VB_WORK)
    for (auto* p : {&v.zpart, &v.z, &v.gN, &v.hN, &v.wN, &v.vN, &v.valpart, &v.tpart}) f(*p);
  if (groups & VB_SAMPLE) {
    f(v.At);
    f(v.stiles);
    sys_buffers(v.ss, f);
  }
  if (groups & VB_PROD) {
    blk_buffers(v.bcsr, f);
    blk_buffers(v.bcsc, f);
  }
  if (groups & VB_CSR) {
    f(v.rowptr);
    f(v.colidx);
    f(v.val);
    blk_buffers(v.sgram, f);
  }
}

}  // namespace scs

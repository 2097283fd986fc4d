// libscsopt: C ABI + per-method step orchestration of the SCORE inner
// iteration on MI355X.  Device work is issued on the context stream; the host
// reads back only the scalars the reference's control flow needs.
//
// Method map (reference -> here):
//   step!(::ProxNSCORE)   prox-N-SCORE.jl:34-119     -> step_newton(NSCORE)
//   step!(::ProxGGNSCORE) prox-GGN-SCORE.jl:34-135   -> step_newton(GGN)
//   step!(::ProxLQNSCORE) prox-L-BFGS-SCORE.jl:69-169 -> step_lqn
//   linesearch / inv_BB_step  utils.jl:27-48           -> line_search / bb kernel
//   get_Mg                    smoothing.jl:12-25        -> get_Mg
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>
#include <execinfo.h>
#include <signal.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/scsopt.h"
#include "common.h"
#include "kernels.h"
#include "batch_plan.h"
#include "data_view.h"
#include "shard_plan.h"

using namespace scs;

namespace {

struct Pending {
  int cat;
  hipEvent_t e0, e1;
};
enum { T_GRAM = 0, T_GEMV, T_SOLVE, T_STEP, T_REDUCE, T_N };
constexpr int ZF_SLOT = 24;   // scal / hscal slot of the deferred f(x) (forward with need_val = false)
// scs_iterate's device-resident loop: f(x) and get_reg(x) of the epoch's x, the norms (3 slots)
constexpr int FX_SLOT = 25, RX_SLOT = 26, NRM_SLOT = 28, LOOP_SLOTS = 32;
constexpr int TF_SLOT = 31;   // ftest(x) of the held-out data (inside LOOP_SLOTS: it rides the loop's hand-off)
constexpr int H0_SLOT = 19;   // the device ring's H0 (scs_iterate's pipelined ProxLQNSCORE loop)

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

}  // namespace

// the data view in place is the ViewData base (data_view.h): the full data, or the view swapped in for
// the duration of a call
struct scs_ctx : ViewData {
  int dev = 0;
  hipStream_t st = nullptr;
  bool own_stream = false;
  std::string err;

  // row sharding: the exchange runs through libscsopt's own RCCL communicator (rccl) or the
  // caller's all-reduce callback (ar); comm_force runs the exchange path at one rank too
  int rank = 0, nranks = 1;
  scs_allreduce_fn ar = nullptr;
  void* ar_user = nullptr;
  ncclComm_t rccl = nullptr;
  bool comm_force = false;
  double* red = nullptr;
  int64_t red_cap = 0;
  bool own_red = false;   // red allocated by the library (no scs_set_reduce_buffer)

  // data
  int64_t m = 0, mpad = 0, row0 = 0;
  // multi-output targets (scs_set_outputs): nout = K outputs share one dense A of dc columns (dcp: padded
  // to whole panels); the variable count is m = dc·K.  nout = 0 (unset): dc = m, dcp = mpad.  The data
  // view's column count (dc, dcp) serves the products, the Gram, the tile lists and the doors; m, mpad
  // everything after the products.
  int nout = 0;
  int64_t dc = 0, dcp = 0;
  // scs_set_sparse_outputs: with nout set the sparse doors are accepted and the products of a sparse A
  // run with K right-hand sides (stored without effect while nout is unset).  ms_kernel: the arm read
  // at the data door (SCS_MULTI_SPARSE_KERNEL / multi_spmm_default): 1 the one-pass kernel on the
  // K-column blocked copies, 0 K launches of the single-vector product on the single-vector copies
  int sparse_outputs = 0;
  int ms_kernel = 0;
  // scs_set_multi_sample: with nout set, ProxGGNSCORE at N·K + 1 <= d·K runs the sample-space branch
  // (multi_sample_direction) instead of being refused (stored without effect while nout is unset)
  int multi_sample = 0;
  // scs_set_multi_batches: with nout set, scs_set_batches accepts a dense A instead of refusing (stored
  // without effect while nout is unset).  mb_gather: the arm read where the list is registered
  // (multi_gather_arm): 1 multi.hip's one-launch gather, 0 gather_rows_kernel over dcp columns plus one
  // launch_gather_y per further target column
  int multi_batches = 0;
  int mb_gather = 1;
  // scs_set_multi_sparse_batches: with nout and multi_batches set, scs_set_batches also accepts a sparse A
  // held in the scs_set_sparse_outputs mode (stored without effect while nout is unset or on a dense A).
  // Its batches are densified views (bpool: the d-column rows through launch_densify_rows, Y_b gathered)
  // or, under ProxLQNSCORE with scs_set_sparse_batches, sparse K-column views (spool).  msb_narrow: the
  // workgroup form of the one-pass kernel on those sparse views, read where the list is registered
  // (multi_narrow_form)
  int multi_sparse_batches = 0;
  int msb_narrow = 0;
  double* mXt = nullptr;   // x = vec(X) repacked K-contiguous (dcp x K, zero beyond dc): launch_multi_pack_x
  double* mVt = nullptr;   // an N x K operand of Aᵀ V repacked K-contiguous (grow-only, mVt_cap doubles)
  int64_t mVt_cap = 0;
  double* Gd = nullptr;    // one dc x dc weighted Gram (dcp²) before its placement into G
  int64_t Nglob_data = 0;   // N_global of the full data (Nglob follows the swapped-in view)
  bool has_data = false;
  bool generic = false;  // ProblemGeneric (no A)
  // fp32 storage of the dense row blocks (scs_set_dense_f32): a32 says what A holds now (it follows the
  // swapped-in view), dense_f32 is the mode of the blocks uploaded or generated next; the arithmetic
  // stays fp64 (f32c below is independent of both)
  int dense_f32 = 0;
  // sparse A: the view's CSR (rows) + the CSC copy (columns) of the full data, values fp64 or fp32
  // scs_set_compute_f32: fp32 ARITHMETIC in the sparse products (fp32-stored values) and the L-BFGS
  // two-loop -- the compute arm of BASELINE configs[4]'s fp32-vs-fp64 study; 0 (fp64) by default
  int f32c = 0;
  int64_t* colptr = nullptr;
  int* rowidx = nullptr;
  void* valT = nullptr;
  SpBlkT bgram;   // the sparse Gram's row copy: 2^sparse_gram_shift()-wide blocks, unpadded (built on first use)
  // scs_set_sparse_sample: ProxGGNSCORE's sample-space P = A diag(h) Aᵀ of a sparse A from its nonzeros
  // (the view's sgram); ssys: the system scratch per size
  int sparse_sample = 0;
  std::vector<SampleSys> ssys;
  struct SegGram {   // the sparse Gram's variant-8 structure (build_gram_seg, on first use)
    int state = 0;   // 0 not tried, 1 built, -1 not built (memory / size): the Gram-blocked walk instead
    int shift = 0;
    uint64_t* seg = nullptr;   // per (block, row) segment records, 8-B units
    uint64_t* T = nullptr;     // per (column, upper block, row of the column): n << 40 | unit
    int64_t* tptr = nullptr;   // T's column offsets
    double* sw = nullptr;      // w[rowidx[p]]·valT[p], per Gram
  } sgseg;
  int sp_gram = 0;   // the Gram of a sparse A: 0 undecided, 1 priced by nnz (sparse_gram_kernel), 2 dense tiles
  double* Ad = nullptr;  // dense panel-blocked mirror of a sparse A (Gram-based methods only)
  // ... or, when the mirror does not fit under the cap, a ring of two R-row dense slots the Gram
  // streams through chunk by chunk (gram_main_stream)
  int sp_mode = 0;              // 0: undecided, 1: mirror, 2: stream
  double* ringA = nullptr;
  int64_t ring_rows = 0;
  int64_t ring_r0[2] = {-1, -1}, ring_n[2] = {0, 0};
  // x-independent Gram reuse (scs_set_gram_cache): Gk holds AᵀQA of data generation gk_gen;
  // data_gen moves on every change of the rows or the loss (new data, batch view swaps)
  int gram_cache = 0;
  double* Gk = nullptr;
  uint64_t data_gen = 1, gk_gen = 0;
  bool g_from_cache = false;   // this step's G was copied from Gk (solve_system)

  // problem
  int loss = 0, ggn = 0;
  double scale = 1.0;
  bool loss_set = false;
  int reg = 0;
  double lam = 0.0, lam2 = 0.0;
  int nlam = 1;
  bool reg_set = false;
  double* clb = nullptr;  // C_set (raw) bounds, length mpad
  double* cub = nullptr;
  int ngroups = 0;
  int* gstart = nullptr;
  int* gend = nullptr;
  double* gw = nullptr;
  double* wel = nullptr;  // per-element group weight (Cmat diagonal)
  int* gmap = nullptr;    // get_P's G, 0-based (null: identity)
  int smooth = 0;
  double mu = 1.0, Mh = 2.0, nu = 2.6;
  bool smooth_set = false;
  double* slb = nullptr;  // sanitized smoother bounds
  double* sub = nullptr;
  bool has_L = false;
  double L = 0.0;

  // method
  int method = 0, ss_type = 1, use_prox = 1, mem = 10;
  bool method_set = false;
  double* S = nullptr;  // [mem+1][mpad]
  double* Yv = nullptr;
  std::vector<int> ring;  // physical slots, oldest -> newest
  int spare = 0;
  int* d_order = nullptr;
  int* hring = nullptr;       // pinned copy of the ring order (asynchronous upload)
  // SCS_LOSS_CALLBACK: the caller's f / grad_fx / hess_fx, with a pinned [x | out] exchange buffer
  scs_loss_fn cb = nullptr;
  void* cb_user = nullptr;
  double* cbh = nullptr;
  size_t cbh_cap = 0;
  int64_t cb_nout = 0;        // rows of the SCS_CB_GGN Jacobian (0: no GGN callback)
  NView cbv;                  // that Jacobian, panel-blocked, swapped in for the GGN step
  double* cbstage = nullptr;  // column-major staging panel for its upload
  // SCS_LOSS_SAMPLEWISE (scs_set_loss_samplewise): the caller's per-sample functions of z = A x and y.
  // swd: device [z scratch | val | d1 | d2 | s], sw_cap doubles each (the largest view seen); swh: the
  // same five areas in pinned host memory (host mode); swy: pinned copies of the views' y (host mode),
  // keyed by the device pointer, the row count and y_stamp, which moves whenever a view's y is
  // (re)written or its buffer could be reused -- y crosses once per view, not once per call
  scs_samplewise_fn* sw = nullptr;
  void* sw_user = nullptr;
  bool sw_dev = false, sw_ggn = false;
  double* swd = nullptr;
  int64_t sw_cap = 0;
  double* swh = nullptr;
  int64_t swh_cap = 0;
  struct SwY {
    const double* key = nullptr;
    int64_t n = -1;
    uint64_t stamp = 0;
    double* h = nullptr;
    int64_t cap = 0;
  } swy[4];
  int swy_next = 0;
  uint64_t y_stamp = 1;
  const double* gfix = nullptr; // scs_step_grad: the caller's ∇fx (device copy) for the step's duration
  bool lbfgs_pending = false; // scs_iterate's device loop: the memory update's dg/gg are read at the epoch end
  int lbfgs_slot = 0;
  double H0 = 1.0;

  // m-space workspace
  double *x = nullptr, *xp = nullptr, *xn = nullptr, *dxv = nullptr, *gr = nullptr, *Hr = nullptr, *hinv = nullptr,
         *zb = nullptr, *d = nullptr, *gq = nullptr, *gqn = nullptr, *gtmp = nullptr, *gtmp2 = nullptr, *q = nullptr,
         *ab = nullptr, *tlwork = nullptr, *scal = nullptr, *gcache[2] = {nullptr, nullptr};
  double* hscal = nullptr;  // pinned host scalars
  int* hserr = nullptr;     // pinned: the one-launch triangular solves' timeout flag, copied after each solve
  double* xstar = nullptr;  // model.x on the device (scs_iterate's rel_error)
  double* lqR = nullptr;    // fused ProxLQNSCORE epoch: LQ_NPART x 256 partial sums
  double* hloop = nullptr;  // pinned: the pipelined loop's per-epoch scalars, two epochs (parity)
  double* hloop_dev = nullptr;   // its device-side address
  hipEvent_t loop_ev[2] = {nullptr, nullptr};
  bool dev_loop = false;    // scs_iterate's device-resident loop: steps leave x_new / pri on the device
  // Gram / solve
  double *G = nullptr, *Gc = nullptr;
  int2* tiles = nullptr;    // Gram launch list
  int ntiles = 0;
  int tall = 0;             // 1: 256 x 128 launch tiles (nb even), packed slots = their 128 x 128 halves
  int2* utiles = nullptr;   // 128 x 128 slot list (unpack)
  int nslots = 0;
  int4* gwork = nullptr;    // tail-balanced schedule (gram_schedule): work items, combine items, partials
  int4* gcomb = nullptr;
  int gseglen = 0, gncomb = 0, gnsplit = 1;
  double* gpart = nullptr;
  // the unpacked launches' list and schedule with the diagonal's D1 blocks paired (gram_tiles.h;
  // null without pairing: SCS_GRAM_DIAGPAIR=0, 128 x 128 tiles, a non-interleaved kernel).  The packed
  // launches (slot = list index) and the strip lists keep `tiles`.
  int2* ptiles = nullptr;
  int nptiles = 0;
  int4* pwork = nullptr;
  int4* pcomb = nullptr;
  int pseglen = 0, pncomb = 0, pnsplit = 1;
  double* vpart = nullptr;   // fused Aᵀv partials: max(gnsplit, strip nsplits, 1) rows of mpad
  // strip pipeline (gram_factor_pipelined): the Gram's tile list cut into the factor's outer
  // strips (tiles with bj in strip s), one tail-balanced schedule each; the factor stream and
  // one event per strip
  struct GStrip {
    int4* work = nullptr;
    int4* comb = nullptr;
    int seglen = 0, nsplit = 1, ncomb = 0;
  };
  std::vector<GStrip> gstrip;
  // the one-launch form (SCS_CHOL_PIPE=2): every strip's tiles in one scheduled launch, each XCD's
  // segment strip-major (its share of strip 0, then of strip 1, ...), K-split pieces in the last
  // strip only; whole tiles count into gp_cnt[strip], gp_target[s] = whole tiles of strip s
  GStrip gpipe;
  std::vector<unsigned> gp_target;
  unsigned* gp_cnt = nullptr;
  int* gp_flag = nullptr;
  int vpieces = 1;           // rows of vpart
  hipStream_t sf = nullptr;
  std::vector<hipEvent_t> evstrip;
  hipEvent_t evfac = nullptr;
  double* W = nullptr;      // inverted diagonal blocks of the Cholesky factor [mpad/128][128*128]
  double* ysol = nullptr;   // triangular-solve scratch (mpad)
  int2* trilist = nullptr;  // row-major lower tiles
  int* cinfo = nullptr;
  CholAux caux;             // two-level factorization constants (chol.hip)
  LUAux lu;                 // blocked LU (lu.hip): the non-SPD fallback and the GGN sample-space system
  // scs_set_solver: SCS_SOLVER_REFERENCE solves the way the reference does -- Householder QR for
  // ProxGGNSCORE's systems (prox-GGN-SCORE.jl:126,131), LU (Julia's `\`) for ProxNSCORE's
  int solver = 0;
  QRAux qr;                 // qr.hip workspace
  double* qrM = nullptr;    // the sample-space system transposed to column-major for the QR
  int64_t qrM_n = 0;
  double* luM = nullptr;    // scs_lu_eval's system / rhs / info, kept so the LU graphs replay
  double* lub = nullptr;
  int* luinfo = nullptr;
  int64_t lu_np = 0;
  // scs_chol_eval's own system, factor workspace and right-hand side (what G, W, ysol, trilist, rbk,
  // cinfo and caux are to a step), sized for the padded order ce_np
  double *ceG = nullptr, *ceW = nullptr, *cey = nullptr, *cerbk = nullptr, *ceb = nullptr;
  int2* cetri = nullptr;
  int* ceinfo = nullptr;
  CholAux ceaux;
  int64_t ce_np = 0;
  // scs_qr_eval's: the row-major staging, the column-major system, the right-hand side, the redo copy
  // and the QR workspace (what Ms, qrM, bS, qbk and qr are to a sample-space step)
  double *qeS = nullptr, *qeA = nullptr, *qeb = nullptr, *qebk = nullptr;
  QRAux qre;
  int64_t qe_np = 0, qebk_n = 0;
  // minibatches (scs_set_batches / scs_select_batch): the collected DataLoader batch list of
  // iterate.jl:141-146 as one device row list; each distinct batch size owns a gathered view
  // (NView) that is swapped in for the steps on that batch
  // On several ranks the list holds GLOBAL row indices: each rank keeps the batch's rows it
  // owns (possibly none) and their positions in the batch (bpos, for the sample-space gather);
  // the batch's global size (bglob) drives the branch choice and the exchange covers the rest.
  int64_t* brows = nullptr;
  std::vector<int64_t> boff;   // batch b = brows[boff[b] .. boff[b + 1]) (local rows)
  std::vector<int64_t> bglob;  // global size of batch b
  std::vector<int64_t> bpos;   // position in its batch of each local row of brows (host)
  std::vector<NView> bpool;    // gathered views, one per distinct (local, global) batch size
  std::vector<int64_t> bheld;  // the batch each pool view currently holds (-1: none)
  int bview = -1;              // the selected batch's pool view (-1: the full data)
  // scs_set_sparse_batches: under ProxLQNSCORE a sparse A's batches are sparse views (spool, one per
  // plan slot: kept per batch within the budget, else one refillable slot per size; batch_plan.h).
  // bscr: grow-only scratch of the view builds, freed with the list.
  int sparse_batches = 0;
  std::vector<NView> spool;
  int spool_kind = 1;          // what spool's views serve: 1 ProxLQNSCORE, 2 ProxGGNSCORE's sample space too
  int vkind = 0;               // the kind of view the method set last asks for (batch_view_kind)
  scs::BatchPlan bplan;
  int spview = -1;             // the selected batch's sparse view (-1: none)
  DevBuf bscr[20];
  int64_t bsel = -1;           // the selected batch (-1: the full data)
  // all ranks' rows of the full data or of the selected batch (GGN sample-space branch with
  // N_global + 1 <= m on several ranks)
  NView gview;
  // held-out data (Problem(...; Atest, ytest), problems.jl:27-28,67-68): a view of its own (VIEW_TEST: rows,
  // y, the f workspace; a sparse set also its CSR + LDS-blocked copy) swapped in only to evaluate
  // ftest(x) = f(Atest, ytest, x) at the loop's stats pushes (iterate.jl:169-175, utils.jl:55-57).
  // `host`: a callback loss evaluates it on the caller's side (SCS_CB_FTEST)
  struct TestSet {
    NView v;
    bool on = false, host = false;
    // exactly one of Atest / ytest given: optim_loop! logs "Will skip testing..." and leaves
    // `ftest` unassigned (iterate.jl:170-171), so its first show_stat! call (:201) raises
    // UndefVarError -- scs_iterate fails the same way at its first stats push
    bool xor_case = false;
    TestSet() { v.parts = VIEW_TEST; }
  } tset;
  bool gview_ok = false;
  int64_t gview_batch = -1;    // the batch gview holds (-1: the full data) ...
  uint64_t gview_gen = 0;      // ... of batch list generation gview_gen
  uint64_t batch_gen = 1;      // bumped whenever the batch list changes (scs_set_batches)
  bool lu_fallback_used = false;
  // the incremental line search's N-space scratch: [z0 | α·A d] trial pair (2 Npad) + A d (Npad)
  double* lsbuf = nullptr;
  int64_t lscap = 0;
  int64_t ls_direct = 0;   // incremental trials re-decided on the direct form (near the Armijo threshold)
  // fallbacks taken instead of failing (scs_fallback_counts): SCS_FB_* in include/scsopt.h
  int64_t fb[SCS_FB_N] = {};
  double* rbk = nullptr;   // (m_pad) the right-hand side before a one-launch solve, for its per-block redo
  double* Gbk = nullptr;   // (m_pad²) the system before a cooperative-panel LU, for its column-step redo
  int64_t Gbk_n = 0;
  double* qbk = nullptr;   // (npad² + npad) A and b before a cooperative-panel QR solve, for its redo
  int64_t qbk_n = 0;

  // caches (CSE of identical evaluations; keyed by the host x content)
  std::vector<double> zkey;
  bool zvalid = false;
  double zfval = 0.0;  // f(x) for zkey (global, scaled)
  bool zf_pending = false;   // zfval still in flight to hscal[8] (forward with need_val = false)
  std::vector<double> gkey[2];
  bool gvalid[2] = {false, false};
  // scs_iterate's host vectors carry version tags (bumped on every write), so the f / ∇q caches
  // compare a tag instead of m doubles and keep no copy; untagged pointers (the per-call ABI)
  // use the content keys above.  A key's tag is 0 for a content key.
  struct XTag {
    const double* p = nullptr;
    uint64_t v = 0;
  } xtags[3];
  uint64_t xtag_next = 1;
  uint64_t ztag = 0, gtag[2] = {0, 0};
  int gnext = 0;

  // the kernels the dominant launches used (scs_kernel_names; rocprofv3's names)
  std::string gram_kname, prod_kname;
  // timing
  bool timing = false;
  int timing_every = 1;     // scs_iterate's pipelined loop: kernel-timing events on every n-th epoch only
  std::vector<Pending> pending;
  double tms[T_N] = {0, 0, 0, 0, 0};
  int64_t tcalls[T_N] = {0, 0, 0, 0, 0};

  std::vector<DevBuf> allocs;

  // a multi-device context (scs_create_multi): one sub-context per device holding its row block
  // (row_plan), one RCCL communicator over the devices (ncclCommInitAll); the entry points a group
  // supports run on every sub-context at once, one host thread each (group_run)
  std::vector<scs_ctx*> subs;
  std::vector<RowBlock> plan;
  int64_t grpN = 0, grpm = 0;   // the whole problem's rows and columns
  bool group_broken = false;
  // one persistent host thread per device (group_run hands each call's per-device work to them:
  // no thread spawn per ABI call); `aborting` is shared with the sub-contexts (comm_abort), which
  // check it before every RCCL call once a failing device has aborted the communicators
  struct Workers;
  std::unique_ptr<Workers> workers;
  std::shared_ptr<std::atomic<bool>> comm_abort;
  // SCS_MULTI_HOST_EXCHANGE groups: the exchange through host memory instead of RCCL
  struct HostExchange;
  std::unique_ptr<HostExchange> hx;
  ~scs_ctx();
};

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
namespace {

struct Fail {
  int code;
};

void set_err(scs_ctx* c, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
}

#define HCK(expr)                                                                                      \
  do {                                                                                                 \
    hipError_t e__ = (expr);                                                                           \
    if (e__ != hipSuccess) {                                                                           \
      set_err(c, "HIP error '%s' at %s:%d (%s)", hipGetErrorString(e__), __FILE__, __LINE__, #expr); \
      throw Fail{SCS_ERR_HIP};                                                                         \
    }                                                                                                  \
  } while (0)

[[noreturn]] void fail(scs_ctx* c, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  c->err = buf;
  throw Fail{code};
}

template <class F>
int guarded(scs_ctx* c, F&& f) {
  if (!c) return SCS_ERR_ARG;
  if (!c->subs.empty()) {   // the group-aware entry points branch to group_* before this
    c->err = "this entry point takes a single-device context (scs_create), not a multi-device one";
    return SCS_ERR_ARG;
  }
  try {
    c->err.clear();
    f();
    return SCS_OK;
  } catch (const Fail& e) {
    return e.code;
  } catch (const std::exception& e) {
    c->err = e.what();
    return SCS_ERR_HIP;
  }
}

// zero = false: the caller's next kernel writes every element (the device door's re-tile)
template <class T>
T* dalloc(scs_ctx* c, size_t n, bool zero = true) {
  void* p = nullptr;
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) fail(c, SCS_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
  if (zero) HCK(hipMemsetAsync(p, 0, bytes, c->st));
  c->allocs.push_back({p, bytes});
  return (T*)p;
}

void dfree(scs_ctx* c, void*& p) {
  if (!p) return;
  for (size_t i = 0; i < c->allocs.size(); ++i)
    if (c->allocs[i].p == p) {
      c->allocs.erase(c->allocs.begin() + i);
      break;
    }
  (void)hipFree(p);
  p = nullptr;
}
template <class T>
void dfree_t(scs_ctx* c, T*& p) {
  void* v = (void*)p;
  dfree(c, v);
  p = nullptr;
}

void h2d(scs_ctx* c, double* dst, const double* src, int64_t n) {
  HCK(hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
}
void d2h(scs_ctx* c, double* dst, const double* src, int64_t n) {
  HCK(hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyDeviceToHost, c->st));
}
// Drain the stream.  A triangular solve whose block wait gave up (~30 s, never expected) flagged
// caux.serr; its copy lands in hserr behind the solve, so the first drain after that solve reports
// it (the step's direction is invalid) instead of the next factor's chain check.
void sync(scs_ctx* c) {
  HCK(hipStreamSynchronize(c->st));
  if (c->hserr && *c->hserr) {
    *c->hserr = 0;
    if (c->caux.serr) HCK(hipMemsetAsync(c->caux.serr, 0, sizeof(int), c->st));
    HCK(hipStreamSynchronize(c->st));
    fail(c, SCS_ERR_HIP, "Cholesky triangular solve: a block wait timed out; this step's direction is invalid");
  }
}

// after a chol_solve on the context stream: its timeout flag -> hserr (checked by sync)
void solve_flag_copy(scs_ctx* c) {
  if (c->hserr && c->caux.serr) HCK(hipMemcpyAsync(c->hserr, c->caux.serr, sizeof(int), hipMemcpyDeviceToHost, c->st));
}

void tbegin(scs_ctx* c, int cat, hipEvent_t* e0) {
  if (!c->timing) return;
  HCK(hipEventCreate(e0));
  HCK(hipEventRecord(*e0, c->st));
  (void)cat;
}
void tend(scs_ctx* c, int cat, hipEvent_t e0) {
  if (!c->timing) return;
  hipEvent_t e1;
  HCK(hipEventCreate(&e1));
  HCK(hipEventRecord(e1, c->st));
  c->pending.push_back({cat, e0, e1});
}
void tresolve(scs_ctx* c) {
  if (c->pending.empty()) return;
  for (auto& p : c->pending) {
    HCK(hipEventSynchronize(p.e1));
    float ms = 0.f;
    HCK(hipEventElapsedTime(&ms, p.e0, p.e1));
    c->tms[p.cat] += ms;
    c->tcalls[p.cat] += 1;
    (void)hipEventDestroy(p.e0);
    (void)hipEventDestroy(p.e1);
  }
  c->pending.clear();
}

// get_Mg (smoothing.jl:12-25)
double get_Mg(scs_ctx* c, double Mh, double nu, double mu, int64_t n) {
  if (Mh < 0) fail(c, SCS_ERR_REF, "Mh must be nonnegative.");
  if (mu <= 0) fail(c, SCS_ERR_REF, "μ must be positive.");
  if (0 < nu && nu <= 3) return std::pow((double)n, (3 - nu) / 2) * std::pow(mu, nu / 2 - 2) * Mh;
  if (nu > 3) return std::pow(mu, 4 - 3 * nu / 2) * Mh;
  fail(c, SCS_ERR_REF, "ν must be positive.");
}

double jl_min_h(double x, double y) {
  auto isless = [](double a, double b) { return (a < b) || (std::signbit(a) && !std::signbit(b)); };
  return (std::isnan(x) || (!std::isnan(y) && isless(x, y))) ? x : y;
}

bool same_x(const std::vector<double>& key, const double* x, int64_t m) {
  return (int64_t)key.size() == m && std::memcmp(key.data(), x, sizeof(double) * m) == 0;
}

uint64_t xtag_of(const scs_ctx* c, const double* x) {
  for (const auto& t : c->xtags)
    if (t.p && t.p == x) return t.v;
  return 0;
}
// cache key (content `key` or tag `ktag`) matches the host vector x; x = nullptr: a device-only
// vector (a line-search trial point) that never hits and is keyed by a fresh tag
bool key_hit(const scs_ctx* c, const std::vector<double>& key, uint64_t ktag, const double* x) {
  if (!x) return false;
  const uint64_t t = xtag_of(c, x);
  if (t) return ktag == t;
  return ktag == 0 && same_x(key, x, c->m);
}
void key_set(scs_ctx* c, std::vector<double>& key, uint64_t& ktag, const double* x) {
  if (!x) {
    key.clear();
    ktag = c->xtag_next++;
    return;
  }
  ktag = xtag_of(c, x);
  if (ktag)
    key.clear();
  else
    key.assign(x, x + c->m);
}

ProxArgsH prox_args(scs_ctx* c) {
  ProxArgsH P;
  P.reg = c->reg;
  P.use_prox = c->use_prox;
  P.lam = c->lam;
  P.lam2 = c->lam2;
  P.lb = c->clb;
  P.ub = c->cub;
  P.gstart = c->gstart;
  P.gend = c->gend;
  P.gw = c->gw;
  P.ngroups = c->ngroups;
  P.gmap = c->gmap;
  return P;
}

void require_ready(scs_ctx* c, bool need_method) {
  if (!c->has_data) fail(c, SCS_ERR_STATE, "no data: call scs_set_data / scs_gen_data first");
  if (!c->loss_set) fail(c, SCS_ERR_STATE, "no loss: call scs_set_loss first");
  if (!c->reg_set) fail(c, SCS_ERR_STATE, "no regularizer: call scs_set_reg first");
  if (need_method && !c->smooth_set) fail(c, SCS_ERR_STATE, "no smoother: call scs_set_smoother first");
  if (need_method && !c->method_set) fail(c, SCS_ERR_STATE, "no method: call scs_method_init first");
}

// the exchange step is active: several ranks, or one rank with the exchange forced
bool sharded(const scs_ctx* c) { return c->nranks > 1 || c->comm_force; }

// scs_set_outputs: K outputs on one A (1 when unset); multi: the multi-output kernels (multi.hip) run
int kout(const scs_ctx* c) { return c->nout ? c->nout : 1; }
bool multi(const scs_ctx* c) { return c->nout >= 2; }
bool multi_loss(int loss) { return loss == SCS_LOSS_SOFTMAX_CE || loss == SCS_LOSS_MULTI_LS; }
// the partials a product on the blocked copy B writes per row (one per group of B.kp blocks)
int blk_groups(const SpBlkT& B) { return (B.nblk + B.kp - 1) / B.kp; }

// doubles of the in-place all-reduce payload: packed Gram tiles ‖ Aᵀv (GGN / NSCORE), the
// m-vector (LQN), or the all-gather of the rows for the sharded GGN sample-space branch
int64_t reduce_buffer_doubles(const scs_ctx* c) {
  const int64_t nb = c->mpad / 128;
  const int64_t tsz = (nb * (nb + 1) / 2 + nb) * 128 * 128;   // 128 x 128 slots (tall lists add <= nb)
  int64_t need = std::max<int64_t>(tsz + c->mpad, c->mpad);
  // GGN sample-space branch across ranks: the all-gather of the rows (Ng x m_pad) and y of the
  // full data when N_global + 1 <= m, and of every registered batch whose global size b has
  // b + 1 <= m -- sized from those sizes, not from m (the buffer outlives view swaps; a new batch
  // list that needs more reallocates a library-owned buffer, scs_set_batches)
  int64_t ng = 0;
  if (c->Nglob_data + 1 <= c->m) ng = c->Nglob_data;
  for (int64_t b : c->bglob)
    if (b + 1 <= c->m) ng = std::max(ng, b);
  if (c->bsel < 0 && c->Nglob + 1 <= c->m) ng = std::max(ng, c->Nglob);
  if (ng > 0) {
    const int64_t Ng = round_up(ng, 16);
    need = std::max<int64_t>(need, Ng * c->mpad + Ng);
  }
  return need + 64;
}

// the payload buffer: the caller's (scs_set_reduce_buffer) or one the library owns
void ensure_red(scs_ctx* c) {
  if (c->red || !sharded(c)) return;
  if (!c->has_data) fail(c, SCS_ERR_STATE, "the reduce buffer needs the data dimensions");
  const int64_t need = reduce_buffer_doubles(c);
  c->red = dalloc<double>(c, need);
  c->red_cap = need;
  c->own_red = true;
}

void allreduce(scs_ctx* c, double* buf, int64_t count) {
  if (!sharded(c)) return;
  if (buf != c->red) fail(c, SCS_ERR_COMM, "internal: all-reduce payload must live in the reduce buffer");
  if (count > c->red_cap) fail(c, SCS_ERR_COMM, "reduce buffer too small (%lld < %lld doubles)",
                               (long long)c->red_cap, (long long)count);
  hipEvent_t e0;
  tbegin(c, T_REDUCE, &e0);
  if (c->comm_abort && c->comm_abort->load(std::memory_order_acquire))
    fail(c, SCS_ERR_COMM, "the multi-device context's communicators were aborted by a failing device");
  // fault injection for the abort path's tests: this rank's exchanges fail (read per call)
  if (const char* fe = std::getenv("SCS_FAULT_EXCHANGE_RANK"))
    if (c->nranks > 1 && std::atoi(fe) == c->rank) fail(c, SCS_ERR_COMM, "injected exchange failure at rank %d", c->rank);
  if (c->rccl) {   // in place, on the context stream (one fp64 sum per exchange)
    const ncclResult_t r = ncclAllReduce(buf, buf, (size_t)count, ncclFloat64, ncclSum, c->rccl, c->st);
    if (r != ncclSuccess) fail(c, SCS_ERR_COMM, "ncclAllReduce: %s", ncclGetErrorString(r));
    // RCCL launches its kernel on c->st, so the events around it time it.  At world 1 the in-place
    // all-reduce launches nothing (0.02 ms, profiles/r05/rccltrace/: no RCCL kernel on any queue);
    // the +7 ms the r04 verdict saw in `solve` with RCCL forced was the factor's two streams sharing
    // one hardware queue once torch and RCCL had created theirs (chol.hip, create_chain_stream).
    // The empty dispatch keeps the end event behind the collective should RCCL ever join c->st by a
    // stream wait instead (an event recorded right after a wait takes the last dispatch's time).
    if (c->timing) HCK(launch_marker(c->st));
  } else {
    if (!c->ar) fail(c, SCS_ERR_COMM, "multi-rank context without a communicator");
    int rc = c->ar(buf, count, (void*)c->st, c->ar_user);
    if (rc != 0) fail(c, SCS_ERR_COMM, "all-reduce callback returned %d", rc);
  }
  tend(c, T_REDUCE, e0);
}

// ---------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------
void alloc_mspace(scs_ctx* c) {
  const int64_t mp = c->mpad;
  double** vs[] = {&c->x, &c->xp, &c->xn, &c->dxv, &c->gr, &c->Hr, &c->hinv, &c->zb, &c->d,
                   &c->gq, &c->gqn, &c->gtmp, &c->gtmp2, &c->q, &c->gcache[0], &c->gcache[1], &c->rbk};
  for (double** v : vs) {
    dfree_t(c, *v);
    *v = dalloc<double>(c, mp);
  }
  dfree_t(c, c->cinfo);
  c->cinfo = dalloc<int>(c, 1);   // factorization info (Cholesky pivot check, LU zero pivot, NaN scan)
  dfree_t(c, c->scal);
  // scalars + the partials of the multi-workgroup tail / L-BFGS update (64..), get_reg (64 + 2·256)
  // and the loop norms (64 + 3·256)
  c->scal = dalloc<double>(c, 64 + 6 * 256);
  dfree_t(c, c->xstar);
  c->xstar = dalloc<double>(c, mp);
  dfree_t(c, c->lqR);
  c->lqR = dalloc<double>(c, (size_t)LQ_NPART * LQ_G);
  dfree_t(c, c->mXt);
  // (16 columns whatever nout: a sparse A's -- or a sparse held-out set's, whose mode may be switched on
  // after this door -- one-pass kernel takes the pack padded to KP <= 16 columns, multi_sparse.hip)
  if (multi(c)) c->mXt = dalloc<double>(c, (size_t)c->dcp * 16);
  if (!c->hscal) HCK(hipHostMalloc((void**)&c->hscal, 64 * sizeof(double), hipHostMallocDefault));
  if (!c->hserr) {
    HCK(hipHostMalloc((void**)&c->hserr, sizeof(int), hipHostMallocDefault));
    *c->hserr = 0;
  }
  if (!c->hloop) {   // written by kernels (lqn_post): fine-grained, device-mapped
    HCK(hipHostMalloc((void**)&c->hloop, 2 * LOOP_SLOTS * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped));
    HCK(hipHostGetDevicePointer((void**)&c->hloop_dev, c->hloop, 0));
  }
}

// free the device buffers of v's groups (data_view.h VB_*)
void free_buffers(scs_ctx* c, ViewData& v, unsigned groups) {
  view_buffers(v, groups, [c](auto*& p) { dfree_t(c, p); });
}

void free_blk(scs_ctx* c, SpBlkT& B) {
  blk_buffers(B, [c](auto*& p) { dfree_t(c, p); });
  B = SpBlkT();
}

// the N-space workspace of v, sized by its rows (a sparse v: by its blocked copies; a sparse held-out
// view brings no column copy and is sized by `bcsc`, the data's)
void alloc_nspace(scs_ctx* c, ViewData& v, const SpBlkT& bcsc) {
  ++c->y_stamp;   // a new view: its y is (re)written by the caller of this function
  const int64_t K = kout(c);   // multi-output: Z, R, P are N x K (stride Npad), the partials K columns per slice
  v.nsplit = v.sparse ? blk_groups(v.bcsr) : gemv_n_splits(v.Npad, c->dc);
  v.nval = epilogue_blocks(v.Npad);
  v.nchunk = v.sparse ? blk_groups(bcsc) : multi(c) ? multi_atv_chunks(v.Npad) : gemv_t_chunks(v.Npad);
  free_buffers(c, v, VB_WORK);
  v.zpart = dalloc<double>(c, (size_t)v.nsplit * v.Npad * K);
  v.z = dalloc<double>(c, v.Npad * K);
  v.gN = dalloc<double>(c, v.Npad * K);
  v.hN = dalloc<double>(c, v.Npad * K);
  v.wN = dalloc<double>(c, v.Npad);
  v.vN = dalloc<double>(c, v.Npad);
  v.valpart = dalloc<double>(c, v.nval);
  v.tpart = dalloc<double>(c, (size_t)v.nchunk * (multi(c) ? c->dcp * K : c->mpad));
}
void alloc_nspace(scs_ctx* c, ViewData& v) { alloc_nspace(c, v, v.bcsc); }
void alloc_nspace(scs_ctx* c) {   // the view in place
  if (!c->generic) alloc_nspace(c, *c);
}

void ensure_gram(scs_ctx* c) {
  if (c->G) return;
  const int64_t mp = c->mpad;
  c->G = dalloc<double>(c, (size_t)mp * mp);
  c->Gc = dalloc<double>(c, (size_t)mp * mp);
  // the Gram's tile lists and schedules cover the data view's columns (one dc x dc block of a
  // multi-output system, placed by launch_multi_place); the solver's lists below the whole system
  if (multi(c)) c->Gd = dalloc<double>(c, (size_t)c->dcp * c->dcp);
  const int nb = (int)(c->dcp / 128);
  std::vector<int2> tl((size_t)nb * (nb + 1) / 2 + nb), ul;
  int nt = 0;
  const char* sq = std::getenv("SCS_GRAM_TALL");
  // 256 x 128 tiles from m = 12288 on (interleaved kernels: C3 73-74 TF/s; at m = 8192 the 128 x 128
  // tiles with 2 workgroups / CU are ~1 % faster, 72.5 vs 71.6 TF/s at C2)
  c->tall = (nb % 2 == 0) && nb >= 96 && !(sq && sq[0] == '0');
  if (sq && sq[0] == '1') c->tall = (nb % 2 == 0);
  if (c->tall) {
    gram_tile_list_tall(nb, tl.data(), &nt);
    ul.resize(2 * (size_t)nt);
    for (int t = 0; t < nt; ++t) {
      ul[2 * t] = make_int2(2 * tl[t].x, tl[t].y);
      ul[2 * t + 1] = make_int2(2 * tl[t].x + 1, tl[t].y);
    }
  } else {
    gram_tile_list(nb, tl.data(), &nt);
    ul.assign(tl.begin(), tl.begin() + nt);
  }
  c->tiles = dalloc<int2>(c, nt);
  HCK(hipMemcpyAsync(c->tiles, tl.data(), sizeof(int2) * nt, hipMemcpyHostToDevice, c->st));
  c->ntiles = nt;
  c->nslots = (int)ul.size();
  std::vector<int2> tp;
  if (c->tall && gram_pair_ok()) {
    int np = 0;
    tp.resize(tl.size());
    gram_tile_list_tall_paired(nb, tp.data(), &np);
    tp.resize(np);
    c->ptiles = dalloc<int2>(c, np);
    HCK(hipMemcpyAsync(c->ptiles, tp.data(), sizeof(int2) * np, hipMemcpyHostToDevice, c->st));
    c->nptiles = np;
  }
  {
    const char* ev = std::getenv("SCS_GRAM_SCHED");
    if (!(ev && ev[0] == '0')) {
      std::vector<int4> wk, cb;
      int npart = 0, npartp = 0;
      // the AV launches' designated tiles first in each XCD's order on 256 x 128 tiles (C3 Gram
      // 3863.7 -> 3846.6 ms); on 128 x 128 tiles it measured slower (C2 Gram +0.3 ms unfused, +0.9 fused;
      // profiles/r05/diagfirst/).  SCS_GRAM_DIAGFIRST=0 / 1: off / also on 128 x 128 tiles (A/B)
      const char* df = std::getenv("SCS_GRAM_DIAGFIRST");
      const int dfg = (df && df[0] == '0') ? 0 : c->tall ? 256 : (df && df[0] == '1') ? 128 : 0;
      c->gseglen = gram_schedule(tl.data(), nt, 32 * (c->tall ? 1 : 2), wk, cb, &c->gnsplit, &npart, dfg);
      c->gncomb = (int)cb.size();
      c->gwork = dalloc<int4>(c, wk.size());
      HCK(hipMemcpyAsync(c->gwork, wk.data(), sizeof(int4) * wk.size(), hipMemcpyHostToDevice, c->st));
      if (c->gncomb > 0) {
        c->gcomb = dalloc<int4>(c, cb.size());
        HCK(hipMemcpyAsync(c->gcomb, cb.data(), sizeof(int4) * cb.size(), hipMemcpyHostToDevice, c->st));
      }
      if (c->ptiles) {   // the same rule on the paired list (its tail, and so its K-split tiles, differ)
        c->pseglen = gram_schedule(tp.data(), c->nptiles, 32, wk, cb, &c->pnsplit, &npartp, dfg);
        c->pncomb = (int)cb.size();
        c->pwork = dalloc<int4>(c, wk.size());
        HCK(hipMemcpyAsync(c->pwork, wk.data(), sizeof(int4) * wk.size(), hipMemcpyHostToDevice, c->st));
        if (c->pncomb > 0) {
          c->pcomb = dalloc<int4>(c, cb.size());
          HCK(hipMemcpyAsync(c->pcomb, cb.data(), sizeof(int4) * cb.size(), hipMemcpyHostToDevice, c->st));
        }
      }
      if (std::max(npart, npartp) > 0)
        c->gpart = dalloc<double>(c, (size_t)std::max(npart, npartp) * (c->tall ? 256 : 128) * 128);
    }
  }
  {
    // the strips of the pipeline: tiles whose column block (bj, 128-wide) lies in outer strip s
    const int OB = chol_outer_block(), ns = (nb + OB - 1) / OB;
    c->gstrip.assign(ns, scs_ctx::GStrip());
    c->vpieces = std::max(std::max(c->gnsplit, c->pnsplit), 1);
    int npart_max = 0;
    for (int s2 = 0; s2 < ns; ++s2) {
      std::vector<int2> st;
      for (int t = 0; t < nt; ++t)
        if (tl[t].y / OB == s2) st.push_back(tl[t]);
      std::vector<int4> wk, cb;
      int nsplit = 1, npart = 0;
      scs_ctx::GStrip& g = c->gstrip[s2];
      g.seglen = gram_schedule(st.data(), (int)st.size(), 32 * (c->tall ? 1 : 2), wk, cb, &nsplit, &npart);
      g.nsplit = nsplit;
      g.ncomb = (int)cb.size();
      g.work = dalloc<int4>(c, wk.size());
      HCK(hipMemcpyAsync(g.work, wk.data(), sizeof(int4) * wk.size(), hipMemcpyHostToDevice, c->st));
      if (!cb.empty()) {
        g.comb = dalloc<int4>(c, cb.size());
        HCK(hipMemcpyAsync(g.comb, cb.data(), sizeof(int4) * cb.size(), hipMemcpyHostToDevice, c->st));
      }
      npart_max = std::max(npart_max, npart);
      c->vpieces = std::max(c->vpieces, nsplit);
    }
    // the one-launch schedule: strips 0 .. ns-2 cut into 8 contiguous per-XCD chunks (no split),
    // the last strip as gram_schedule lays it out (tail pieces + combine items)
    {
      const int slots = 32 * (c->tall ? 1 : 2);
      std::vector<std::vector<int4>> seg(8);
      c->gp_target.assign(ns, 0u);
      std::vector<int4> cbl;
      int nsplit = 1, npart = 0;
      for (int s2 = 0; s2 < ns; ++s2) {
        std::vector<int2> st;
        std::vector<int> ix;
        for (int t = 0; t < nt; ++t)
          if (tl[t].y / OB == s2) {
            st.push_back(tl[t]);
            ix.push_back(t);
          }
        const int n = (int)st.size();
        if (s2 + 1 < ns) {
          c->gp_target[s2] = (unsigned)n;
          const int q = n / 8, r = n % 8;
          int t0 = 0;
          for (int x = 0; x < 8; ++x) {
            const int nx = q + (x < r ? 1 : 0);
            for (int i = 0; i < nx; ++i) seg[x].push_back(make_int4(st[t0 + i].x, st[t0 + i].y, -1, ix[t0 + i]));
            t0 += nx;
          }
        } else {
          std::vector<int4> wk;
          const int sl = gram_schedule(st.data(), n, slots, wk, cbl, &nsplit, &npart);
          for (int x = 0; x < 8; ++x)
            for (int i = 0; i < sl; ++i) {
              int4 it = wk[(size_t)x * sl + i];
              if (it.x < 0) continue;
              if (it.z < 0) it.w = ix[it.w];   // whole tile: its canonical index
              seg[x].push_back(it);
            }
          for (auto& cb : cbl) cb.z = ix[cb.z];
        }
      }
      size_t seglen = 0;
      for (auto& v : seg) seglen = std::max(seglen, v.size());
      std::vector<int4> wk(8 * seglen, make_int4(-1, -1, -1, -1));
      for (int x = 0; x < 8; ++x)
        for (size_t i = 0; i < seg[x].size(); ++i) wk[x * seglen + i] = seg[x][i];
      scs_ctx::GStrip& g = c->gpipe;
      g.seglen = (int)seglen;
      g.nsplit = nsplit;
      g.ncomb = (int)cbl.size();
      g.work = dalloc<int4>(c, wk.size());
      HCK(hipMemcpyAsync(g.work, wk.data(), sizeof(int4) * wk.size(), hipMemcpyHostToDevice, c->st));
      if (!cbl.empty()) {
        g.comb = dalloc<int4>(c, cbl.size());
        HCK(hipMemcpyAsync(g.comb, cbl.data(), sizeof(int4) * cbl.size(), hipMemcpyHostToDevice, c->st));
      }
      npart_max = std::max(npart_max, npart);
      c->vpieces = std::max(c->vpieces, nsplit);
      c->gp_cnt = dalloc<unsigned>(c, ns);
      c->gp_flag = dalloc<int>(c, 1);
      HCK(hipMemsetAsync(c->gp_flag, 0, sizeof(int), c->st));
    }
    if (npart_max > 0) {
      const size_t need = (size_t)npart_max * (c->tall ? 256 : 128) * 128;
      // gpart is shared with the one-launch schedule: size it for the larger user
      size_t have = 0;
      for (auto& a : c->allocs)
        if (a.p == c->gpart) have = a.bytes / sizeof(double);
      if (need > have) {
        if (c->gpart) dfree_t(c, c->gpart);
        c->gpart = dalloc<double>(c, need);
      }
    }
  }
  c->vpart = dalloc<double>(c, (size_t)c->vpieces * mp);
  c->utiles = dalloc<int2>(c, ul.size());
  HCK(hipMemcpyAsync(c->utiles, ul.data(), sizeof(int2) * ul.size(), hipMemcpyHostToDevice, c->st));
  {
    const int nb2 = (int)(mp / 128);
    c->W = dalloc<double>(c, (size_t)mp * 128);
    c->ysol = dalloc<double>(c, mp);
    std::vector<int2> tr((size_t)nb2 * (nb2 + 1) / 2);
    gram_tile_list_rowmajor(nb2, tr.data());
    c->trilist = dalloc<int2>(c, tr.size());
    HCK(hipMemcpyAsync(c->trilist, tr.data(), sizeof(int2) * tr.size(), hipMemcpyHostToDevice, c->st));
    HCK(chol_aux_init(&c->caux, mp, c->st));
  }
  sync(c);
}

void invalidate_caches(scs_ctx* c) {
  c->zvalid = false;
  c->zf_pending = false;
  c->gvalid[0] = c->gvalid[1] = false;
}

// ---------------------------------------------------------------------------
// f / ∇f building blocks
// ---------------------------------------------------------------------------
// finalize a loss sum: the per-kind constant of f (see epilogue_kernel)
// a panel-blocked block of `rows` (padded) rows: bytes, and its allocation (a float block is kept
// in the double-typed field, rows * mpad / 2 doubles; mpad % 128 == 0)
size_t a_block_bytes(const scs_ctx* c, int64_t rows, int a32) {
  return (size_t)rows * c->dcp * (a32 ? sizeof(float) : sizeof(double));
}
double* alloc_A(scs_ctx* c, int64_t rows, int a32, bool zero = true) {
  return dalloc<double>(c, a_block_bytes(c, rows, a32) / sizeof(double), zero);
}

// exchange the context's N-dependent fields with v (the full data <-> a minibatch)
void swap_view(scs_ctx* c, NView& v) {
  ++c->data_gen;
  swap_view_data(*c, v, v.parts);
}

// give v's buffers back and reset its fields (what it carries, v.parts, stays)
void free_view(scs_ctx* c, NView& v) {
  ++c->y_stamp;   // a later allocation may reuse y's address
  free_buffers(c, v, VB_ALL);
  static_cast<ViewData&>(v) = ViewData();
}

void free_sample_sys(scs_ctx* c) {
  for (SampleSys& S : c->ssys) sys_buffers(S, [c](auto*& p) { dfree_t(c, p); });
  c->ssys.clear();
}

// 0: dense batch views, 1: sparse views for ProxLQNSCORE, 2: sparse views for ProxGGNSCORE's batches
// with n_b + 1 <= m (dense ones for the rest) -- one rank only: the sharded sample branch needs a dense A
// A multi-output context (scs_set_multi_sparse_batches): 1 for ProxLQNSCORE (sparse K-column views), else
// 0 (densified views); never 2 -- scs_set_sparse_sample stays without effect there.
int batch_view_kind(const scs_ctx* c, int method) {
  if (!c->sparse_batches || !c->sparse) return 0;
  if (method == SCS_PROX_LQNSCORE) return 1;
  if (multi(c)) return 0;
  if (method == SCS_PROX_GGNSCORE && c->sparse_sample && !sharded(c)) return 2;
  return 0;
}

// the held-out view <-> the context's data fields (f's fields only: rows, y, the products'
// workspace and, for a sparse set, the CSR arrays and the SpMV's blocked copy).  Not a data
// change: the data generation (the Gram cache's key) and the product kernel name are kept.
void swap_test(scs_ctx* c) {
  const uint64_t gen = c->data_gen;
  swap_view(c, c->tset.v);
  c->data_gen = gen;
}

struct TestScope {
  scs_ctx* c;
  std::string pk;
  explicit TestScope(scs_ctx* cc) : c(cc), pk(cc->prod_kname) { swap_test(c); }
  ~TestScope() {
    swap_test(c);
    c->prod_kname = pk;
  }
};

void free_test(scs_ctx* c) {
  auto& t = c->tset;
  free_view(c, t.v);
  t.on = t.host = t.xor_case = false;
}

// scs_step on the selected minibatch view: swapped in (and the data-keyed caches dropped) for
// the call, swapped back even when the step fails
struct BatchScope {
  scs_ctx* c;
  int k, ks;   // the dense pool view or the sparse view (at most one is >= 0)
  explicit BatchScope(scs_ctx* cc) : c(cc), k(cc->bview), ks(cc->spview) { swap(); }
  ~BatchScope() { swap(); }
  void swap() {
    if (k < 0 && ks < 0) return;
    swap_view(c, ks >= 0 ? c->spool[ks] : c->bpool[k]);
    invalidate_caches(c);
  }
};

void unselect_view(scs_ctx* c) { c->bview = c->spview = -1; }

// the sparse views and the scratch of their builds (the registered list stays)
void free_sparse_views(scs_ctx* c) {
  for (NView& v : c->spool) free_view(c, v);
  c->spool.clear();
  c->bplan.slots.clear();
  c->bplan.kept_bytes = 0;
  c->spview = -1;
  for (DevBuf& b : c->bscr) {
    dfree(c, b.p);
    b.bytes = 0;
  }
}

void free_dense_views(scs_ctx* c) {
  for (NView& v : c->bpool) free_view(c, v);
  c->bpool.clear();
  c->bheld.clear();
  c->bview = -1;
}

void clear_batches(scs_ctx* c) {
  // the gathered rows of a batch index belong to the list they came from: a new list (a
  // reshuffle, another slice) must not reuse them
  ++c->batch_gen;
  if (c->gview_ok && c->gview_batch >= 0) {
    free_view(c, c->gview);
    c->gview_ok = false;
  }
  free_dense_views(c);
  free_sparse_views(c);
  free_sample_sys(c);
  c->bplan.reset(0);
  c->boff.clear();
  c->bglob.clear();
  c->bpos.clear();
  dfree_t(c, c->brows);
  c->bview = -1;
  c->bsel = -1;
}

// ---- sparse batch views (scs_set_sparse_batches) ----------------------------------------
size_t alloc_bytes(const scs_ctx* c, const void* p) {
  if (p)
    for (const DevBuf& a : c->allocs)
      if (a.p == p) return a.bytes;
  return 0;
}

// device bytes of a sparse view: y, the sample-space workspace and the two blocked copies (a view for
// the GGN sample space: also its plain CSR and the Gram-blocked column copy)
int64_t sparse_view_bytes(const scs_ctx* c, const NView& v) {
  size_t t = 0;
  view_buffers(v, VB_SPARSE_VIEW, [&](const void* p) { t += alloc_bytes(c, p); });
  return (int64_t)t;
}

// bytes the context's sparse data takes (the full data in place): the default budget of the kept views
int64_t sparse_data_bytes(const scs_ctx* c) {
  size_t t = 0;
  for (const void* p : {(const void*)c->rowptr, (const void*)c->colptr, (const void*)c->colidx,
                        (const void*)c->rowidx, (const void*)c->val, (const void*)c->valT,
                        (const void*)c->bcsr.ptr, (const void*)c->bcsr.lidx, (const void*)c->bcsr.val,
                        (const void*)c->bcsc.ptr, (const void*)c->bcsc.lidx, (const void*)c->bcsc.val})
    t += alloc_bytes(c, p);
  return (int64_t)t;
}

// scratch k of the view builds: at least n elements, contents undefined.  Grow-only while the batch
// list lives, so a steady sequence of builds allocates nothing but the views' own arrays (§2d: the
// stalls of a build are its hipMalloc calls).
enum { BS_CNTR = 0, BS_PTRR, BS_RCNT, BS_RPTR, BS_IDX, BS_VAL, BS_CCNT, BS_RANK, BS_COLPTR, BS_ROWIDX, BS_VALT,
       BS_ROWIDX_S, BS_VALT_S, BS_BCNT, BS_BFIRST, BS_PTRC, BS_TMP, BS_GCNT, BS_GFIRST, BS_GPTR, BS_N };
template <class T>
T* bscratch(scs_ctx* c, int k, size_t n) {
  static_assert(BS_N <= sizeof(c->bscr) / sizeof(c->bscr[0]), "scratch slots");
  DevBuf& b = c->bscr[k];
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  if (b.bytes < bytes) {
    dfree(c, b.p);
    b.bytes = 0;
    b.p = dalloc<char>(c, bytes, false);
    b.bytes = bytes;
  }
  return (T*)b.p;
}

// The sparse view of batch b: bit for bit the bcsr / bcsc that scs_set_sparse builds from
// A[rows_b, :] (rows in batch order, batch positions as row numbers), y[rows_b] and a workspace of
// its own.  Row side: a slice of the full row copy (sparse.hip blk_slice_*).  Column side: the
// batch's CSR rows gathered, transposed as the device door transposes (csr_claim / csr_place),
// sorted per column and blocked as build_blocked does -- on scratch, two read-backs of sizes.
// ssv (ProxGGNSCORE's sample space, scs_set_sparse_sample): the view also keeps the gathered CSR rows and
// the Gram-blocked copy of its CSC -- colptr_b / rowidx_s / valT_s cut into 2^sparse_gram_shift()-wide
// blocks of batch positions, unpadded, as build_gram_blocked cuts the rows.
// A multi-output context (scs_set_multi_sparse_batches): the columns are the data view's
// (dc / dcp, not the variable count), the row side keeps the full copy's sub-block shift and kp, the
// column side is cut at multi_spmm_shift(n_b, K) on the product-kernel arm (kp sub-blocks per partial)
// and at spmv_blk_shift(n_b) on the loop arm, the K columns of Y are gathered and the workspace holds
// one partial per (group, column).  Both copies carry the workgroup form of the one-pass kernel.
// Returns the view's slot in spool / bplan.
int build_sparse_view(scs_ctx* c, int64_t b, bool ssv) {
  const int64_t n = c->boff[b + 1] - c->boff[b], ng = c->bglob[b];
  const int64_t* rows = c->brows + c->boff[b];
  const int64_t N = c->N, m = c->dc;   // (dc = the variable count unless nout is set)
  const int64_t K = kout(c);
  const int f32 = c->sp_f32;
  const size_t vs = f32 ? sizeof(float) : sizeof(double);
  const SpBlkT& F = c->bcsr;
  NView v;
  v.parts = ssv ? VIEW_SPARSE_SAMPLE : VIEW_SPARSE;
  v.sparse = true;
  v.N = n;
  v.Nglob = ng;
  // a rank that owns none of the batch's rows keeps one zero stage of workspace (N = 0, nnz = 0: the
  // products launch nothing and its zero partials add nothing to the exchanged sums)
  v.Npad = round_up(std::max<int64_t>(n, 1), 16);
  v.nstage = v.Npad / 16;
  SpBlkT &R = v.bcsr, &Cc = v.bcsc;   // owned by v from the start: free_view gives a failed build's arrays back
  R.shift = F.shift;
  R.nblk = F.nblk;
  R.kp = F.kp;
  Cc.kp = c->bcsc.kp;
  Cc.shift = Cc.kp > 1 ? multi_spmm_shift(n, c->nout) : spmv_blk_shift(n);
  Cc.nblk = (int)std::max<int64_t>(ceil_div(n, int64_t(1) << Cc.shift), 1);
  R.narrow = Cc.narrow = (multi(c) && F.kp > 1) ? c->msb_narrow : 0;
  const int64_t nkR = (int64_t)R.nblk * n, nkC = (int64_t)Cc.nblk * m;
  int64_t nnzpR = 0, nnzb = 0, nnzpC = 0;
  int64_t *ptrR = nullptr, *ptrC = nullptr, *colptr_b = nullptr, *bfirst = nullptr;
  int* rowidx_s = nullptr;
  void* valT_s = nullptr;
  SpBlkT& Gb = v.sgram;   // (ssv)
  Gb.shift = sparse_gram_shift();
  Gb.nblk = (int)std::max<int64_t>(ceil_div(n, int64_t(1) << Gb.shift), 1);
  const int64_t nkG = (int64_t)Gb.nblk * m;
  int64_t *rptr_s = nullptr, *gfirst = nullptr, *gptr = nullptr;
  int* idx_s = nullptr;
  void* val_s = nullptr;
  auto scan = [&](const int64_t* cnt, int64_t* out, int64_t cntn) {
    size_t tb = 0;
    HCK(blk_scan(nullptr, &tb, cnt, out, cntn, c->st));
    void* tmp = bscratch<char>(c, BS_TMP, tb);
    HCK(blk_scan(tmp, &tb, cnt, out, cntn, c->st));
  };
  if (n > 0) {
    int64_t* cntR = bscratch<int64_t>(c, BS_CNTR, nkR + 1);
    ptrR = bscratch<int64_t>(c, BS_PTRR, nkR + 1);
    int64_t* rcnt = bscratch<int64_t>(c, BS_RCNT, n + 1);
    int64_t* rptr = bscratch<int64_t>(c, BS_RPTR, n + 1);
    rptr_s = rptr;
    HCK(blk_slice_size(F.ptr, N, rows, n, R.nblk, cntR, c->st));
    HCK(csr_rows_size(c->rowptr, rows, n, rcnt, c->st));
    scan(cntR, ptrR, nkR + 1);
    scan(rcnt, rptr, n + 1);
    HCK(hipMemcpyAsync(&nnzpR, ptrR + nkR, sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
    HCK(hipMemcpyAsync(&nnzb, rptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
    sync(c);
    // the segmented sort counts its items in an int; the transposition's ranks are 32 bits wide
    if (nnzb > (int64_t)INT32_MAX)
      fail(c, SCS_ERR_ARG, "sparse batch %lld holds %lld entries (a sparse view takes at most 2^31 - 1)", (long long)b,
           (long long)nnzb);
    colptr_b = bscratch<int64_t>(c, BS_COLPTR, m + 1);
    rowidx_s = bscratch<int>(c, BS_ROWIDX_S, nnzb);
    valT_s = bscratch<char>(c, BS_VALT_S, (size_t)nnzb * vs);
    if (nnzb > 0) {
      int* idx_b = bscratch<int>(c, BS_IDX, nnzb);
      void* val_b = bscratch<char>(c, BS_VAL, (size_t)nnzb * vs);
      int64_t* ccnt = bscratch<int64_t>(c, BS_CCNT, m + 1);
      uint32_t* rank = bscratch<uint32_t>(c, BS_RANK, nnzb);
      int* rowidx_b = bscratch<int>(c, BS_ROWIDX, nnzb);
      void* valT_b = bscratch<char>(c, BS_VALT, (size_t)nnzb * vs);
      idx_s = idx_b;
      val_s = val_b;
      HCK(csr_rows_gather(c->rowptr, c->colidx, c->val, f32, rows, n, rptr, idx_b, val_b, c->st));
      HCK(hipMemsetAsync(ccnt, 0, sizeof(int64_t) * (m + 1), c->st));
      HCK(csr_claim(rptr, idx_b, n, ccnt, rank, c->st));
      scan(ccnt, colptr_b, m + 1);
      HCK(csr_place(rptr, idx_b, val_b, f32, n, colptr_b, rank, rowidx_b, valT_b, c->st));
      int end_bit = 1;   // build_blocked's key width for n "columns" (the batch positions)
      while ((int64_t(1) << end_bit) < n) ++end_bit;
      size_t tb = 0;
      HCK(sort_segments(nullptr, &tb, rowidx_b, rowidx_s, valT_b, valT_s, f32, nnzb, m, colptr_b, end_bit, c->st));
      void* tmp = bscratch<char>(c, BS_TMP, tb);
      HCK(sort_segments(tmp, &tb, rowidx_b, rowidx_s, valT_b, valT_s, f32, nnzb, m, colptr_b, end_bit, c->st));
    } else {
      HCK(hipMemsetAsync(colptr_b, 0, sizeof(int64_t) * (m + 1), c->st));
    }
    int64_t* bcnt = bscratch<int64_t>(c, BS_BCNT, nkC + 1);
    bfirst = bscratch<int64_t>(c, BS_BFIRST, nkC + 1);
    ptrC = bscratch<int64_t>(c, BS_PTRC, nkC + 1);
    HCK(hipMemsetAsync(bcnt, 0, sizeof(int64_t) * (nkC + 1), c->st));
    HCK(blk_count(colptr_b, rowidx_s, m, Cc.shift, bcnt, bfirst, c->st));
    HCK(blk_pad(bcnt, nkC, f32, c->st));
    scan(bcnt, ptrC, nkC + 1);
    HCK(hipMemcpyAsync(&nnzpC, ptrC + nkC, sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
    if (ssv) {   // the unpadded cut of the same columns: it holds the batch's nnzb entries
      int64_t* gcnt = bscratch<int64_t>(c, BS_GCNT, nkG + 1);
      gfirst = bscratch<int64_t>(c, BS_GFIRST, nkG + 1);
      gptr = bscratch<int64_t>(c, BS_GPTR, nkG + 1);
      HCK(hipMemsetAsync(gcnt, 0, sizeof(int64_t) * (nkG + 1), c->st));
      HCK(blk_count(colptr_b, rowidx_s, m, Gb.shift, gcnt, gfirst, c->st));
      scan(gcnt, gptr, nkG + 1);
    }
    sync(c);
  }
  // the view's bytes from its shapes (dalloc's sizes), to choose its slot before anything is allocated:
  // a refillable slot gives its old view back first
  const int nval = epilogue_blocks(v.Npad);
  auto ab = [](int64_t cnt, size_t eb) { return (int64_t)(std::max<int64_t>(cnt, 1) * (int64_t)eb); };
  const int64_t nR = n > 0 ? nkR + 1 : 1, nC = n > 0 ? nkC + 1 : 1;
  const int64_t nG = n > 0 ? nkG + 1 : 1;
  // (y, z, gN, hN: K columns each; wN, vN; zpart and tpart: one partial per (group, column))
  const int64_t bytes = ab(v.Npad * K, 8) * 4 + ab(v.Npad, 8) * 2 + ab((int64_t)blk_groups(R) * v.Npad * K, 8) +
                        ab(nval, 8) + ab((int64_t)blk_groups(Cc) * c->dcp * K, 8) + ab(nR, 8) + ab(nC, 8) +
                        ab(nnzpR + 8, 2) +
                        ab(nnzpR + 8, vs) + ab(nnzpC + 8, 2) + ab(nnzpC + 8, vs) +
                        (ssv ? ab(n + 1, 8) + ab(nnzb, 4) + ab(nnzb, vs) + ab(nG, 8) + ab(nnzb + 8, 2) +
                                   ab(nnzb + 8, vs)
                             : 0);
  const int old = c->bplan.refill_target(n, ng, bytes);
  if (old >= 0) {
    free_view(c, c->spool[old]);
    c->bplan.slots[old].batch = -1;
    c->bplan.slots[old].bytes = 0;
  }
  struct Guard {   // a failed build leaves no half-made view behind
    scs_ctx* c;
    NView* v;
    bool done = false;
    ~Guard() {
      if (!done) free_view(c, *v);
    }
  } guard{c, &v};
  const int pad = spmv_pad_index();
  R.ptr = dalloc<int64_t>(c, nR, n == 0);
  R.lidx = dalloc<uint16_t>(c, nnzpR + 8, false);
  R.val = f32 ? (void*)dalloc<float>(c, nnzpR + 8, false) : (void*)dalloc<double>(c, nnzpR + 8, false);
  // the +8 tail reads as pad index / zero, as build_blocked leaves it
  HCK(hipMemsetD16Async((hipDeviceptr_t)(R.lidx + nnzpR), (unsigned short)pad, 8, c->st));
  HCK(hipMemsetAsync((char*)R.val + (size_t)nnzpR * vs, 0, 8 * vs, c->st));
  Cc.ptr = dalloc<int64_t>(c, nC, n == 0);
  Cc.lidx = dalloc<uint16_t>(c, nnzpC + 8, false);
  HCK(hipMemsetD16Async((hipDeviceptr_t)Cc.lidx, (unsigned short)pad, (size_t)(nnzpC + 8), c->st));
  Cc.val = f32 ? (void*)dalloc<float>(c, nnzpC + 8) : (void*)dalloc<double>(c, nnzpC + 8);
  v.y = dalloc<double>(c, v.Npad * K, false);
  for (int64_t l = 0; l < K; ++l)   // Y_b: n_b x K with stride Npad_b
    HCK(launch_gather_y(c->y + l * c->Npad, rows, n, v.Npad, v.y + l * v.Npad, c->st));
  if (n > 0) {
    HCK(hipMemcpyAsync(R.ptr, ptrR, sizeof(int64_t) * nR, hipMemcpyDeviceToDevice, c->st));
    HCK(hipMemcpyAsync(Cc.ptr, ptrC, sizeof(int64_t) * nC, hipMemcpyDeviceToDevice, c->st));
    HCK(blk_slice_copy(F.ptr, F.lidx, F.val, f32, N, rows, n, R.nblk, R.ptr, R.lidx, R.val, c->st));
    HCK(blk_scatter(colptr_b, rowidx_s, valT_s, f32, m, Cc.shift, Cc.ptr, bfirst, Cc.lidx, Cc.val, c->st));
  }
  if (ssv) {
    v.rowptr = dalloc<int64_t>(c, n + 1, n == 0);
    v.colidx = dalloc<int>(c, nnzb, false);
    v.val = dalloc<char>(c, (size_t)std::max<int64_t>(nnzb, 1) * vs, false);
    Gb.nnz = nnzb;
    Gb.ptr = dalloc<int64_t>(c, nG, n == 0);
    Gb.lidx = dalloc<uint16_t>(c, nnzb + 8, false);
    Gb.val = dalloc<char>(c, (size_t)(nnzb + 8) * vs, false);
    // the +8 tail is read (never added) by the walks' idle lanes
    HCK(hipMemsetAsync(Gb.lidx + nnzb, 0, 8 * sizeof(uint16_t), c->st));
    HCK(hipMemsetAsync((char*)Gb.val + (size_t)nnzb * vs, 0, 8 * vs, c->st));
    if (n > 0) {
      HCK(hipMemcpyAsync(v.rowptr, rptr_s, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToDevice, c->st));
      HCK(hipMemcpyAsync(Gb.ptr, gptr, sizeof(int64_t) * nG, hipMemcpyDeviceToDevice, c->st));
    }
    if (nnzb > 0) {
      HCK(hipMemcpyAsync(v.colidx, idx_s, sizeof(int) * nnzb, hipMemcpyDeviceToDevice, c->st));
      HCK(hipMemcpyAsync(v.val, val_s, (size_t)nnzb * vs, hipMemcpyDeviceToDevice, c->st));
      HCK(blk_scatter(colptr_b, rowidx_s, valT_s, f32, m, Gb.shift, Gb.ptr, gfirst, Gb.lidx, Gb.val, c->st));
    }
  } else {
    Gb = SpBlkT();
  }
  v.nnz = nnzb;
  alloc_nspace(c, v);   // the workspace follows the view's nblk (nsplit / nchunk)
  sync(c);
  guard.done = true;
  bool fresh = false;
  const int k = c->bplan.place(b, n, ng, bytes, &fresh);
  // the slot carries the bytes as allocated (they are `bytes` unless dalloc's sizes change)
  const int64_t actual = sparse_view_bytes(c, v);
  if (c->bplan.slots[k].kept) c->bplan.kept_bytes += actual - bytes;
  c->bplan.slots[k].bytes = actual;
  if (fresh) c->spool.push_back(v);
  else c->spool[k] = v;
  c->spool_kind = ssv ? 2 : 1;
  return k;
}

// select batch b (-1: the full data) for the following steps: its size's pool view is
// allocated on first use (A / y rows + the sample-space workspace sized by its own Npad)
// and re-gathered only when it holds another batch.  With scs_set_sparse_batches on, a sparse A
// under ProxLQNSCORE gets the batch's sparse view instead: kept per batch within the budget, else
// rebuilt into the refillable slot of its size (batch_plan.h).
void select_batch(scs_ctx* c, int64_t b, bool dense_view = false) {   // dense_view: scs_get_batch_data's read
  unselect_view(c);
  c->bsel = b < 0 ? -1 : b;
  if (b < 0) return;
  // f(A, y, x) = 1/2 x'(A x) + y'x reads A as an m x m operator, not as samples
  if (c->loss == SCS_LOSS_QUADRATIC) fail(c, SCS_ERR_ARG, "the quadratic loss has no samples to batch");
  const int64_t n = c->boff[b + 1] - c->boff[b], ng = c->bglob[b];
  const int kind = (c->method_set && !dense_view) ? batch_view_kind(c, c->method) : 0;
  if (!dense_view) c->vkind = kind;
  // (kind 2: a batch of the feature branch, n_b + 1 > m, keeps the dense view and the m x m Gram)
  if (kind == 1 || (kind == 2 && ng + 1 <= c->m)) {
    int ks = c->bplan.find(b);
    if (ks < 0) ks = build_sparse_view(c, b, kind == 2);
    c->spview = ks;
    return;
  }
  int k = -1;
  for (int i = 0; i < (int)c->bpool.size(); ++i)
    if (c->bpool[i].N == n && c->bpool[i].Nglob == ng) k = i;
  if (k < 0) {
    NView v;
    v.N = n;
    v.Nglob = ng;
    // a rank that owns none of the batch's rows keeps one zero 16-row stage (the kernels mask
    // rows >= N, so it contributes nothing to the exchanged sums)
    v.Npad = round_up(std::max<int64_t>(n, 1), 16);
    v.nstage = v.Npad / 16;
    v.a32 = c->sparse ? 0 : c->a32;   // a batch of an fp32-stored A is fp32; the dense batch of a sparse A fp64
    v.A = alloc_A(c, v.Npad, v.a32);
    v.y = dalloc<double>(c, v.Npad * kout(c));   // a multi-output view: Y_b, n_b x K with stride Npad_b
    alloc_nspace(c, v);
    c->bpool.push_back(v);
    c->bheld.push_back(-1);
    k = (int)c->bpool.size() - 1;
  }
  if (c->bheld[k] != b) {
    NView& v = c->bpool[k];
    ++c->y_stamp;   // the view's y is gathered again
    if (n == 0) {
      HCK(hipMemsetAsync(v.A, 0, a_block_bytes(c, v.Npad, v.a32), c->st));
      HCK(hipMemsetAsync(v.y, 0, sizeof(double) * v.Npad * kout(c), c->st));
    } else if (multi(c) && c->sparse) {   // scs_set_multi_sparse_batches: Matrix(As') of the d-column rows, Y_b
      const int64_t* rows = c->brows + c->boff[b];
      HCK(hipMemsetAsync(v.A, 0, a_block_bytes(c, v.Npad, 0), c->st));
      HCK(launch_densify_rows(c->rowptr, c->colidx, c->val, c->sp_f32, rows, n, v.Npad, c->y, v.A, v.y, c->st));
      for (int l = 1; l < c->nout; ++l)
        HCK(launch_gather_y(c->y + (int64_t)l * c->Npad, rows, n, v.Npad, v.y + (int64_t)l * v.Npad, c->st));
    } else if (multi(c)) {   // scs_set_multi_batches (a dense A): dcp columns and the K target columns
      const int64_t* rows = c->brows + c->boff[b];
      if (c->mb_gather) {
        HCK(launch_multi_gather_rows(c->A, c->a32, c->Npad, c->dcp, c->y, c->Npad, c->nout, rows, n, v.Npad, v.A, v.y,
                                     c->st));
      } else {
        HCK(launch_gather_rows(c->A, c->a32, c->Npad, c->y, rows, n, v.Npad, c->dcp, v.A, v.a32, v.y, c->st));
        for (int l = 1; l < c->nout; ++l)
          HCK(launch_gather_y(c->y + (int64_t)l * c->Npad, rows, n, v.Npad, v.y + (int64_t)l * v.Npad, c->st));
      }
    } else if (c->sparse) {   // CSR rows -> the dense batch (the reference's Matrix(As') of a sparse A)
      HCK(hipMemsetAsync(v.A, 0, sizeof(double) * (size_t)v.Npad * c->mpad, c->st));
      HCK(launch_densify_rows(c->rowptr, c->colidx, c->val, c->sp_f32, c->brows + c->boff[b], n, v.Npad, c->y,
                              v.A, v.y, c->st));
    } else {
      HCK(launch_gather_rows(c->A, c->a32, c->Npad, c->y, c->brows + c->boff[b], n, v.Npad, c->mpad, v.A, v.a32, v.y,
                             c->st));
    }
    // the view's GGN sample-space Aᵀ copy (built once per A, ggn_sample_step) follows its rows
    // (a multi-output view's copy has the data view's dc columns: multi_sample_setup)
    if (v.At) HCK(launch_transpose(v.A, v.a32, v.Npad, n, c->dc, v.At, c->dcp, v.ss.NpS, c->st));
    c->bheld[k] = b;
  }
  c->bview = k;
}

double loss_scale_value(scs_ctx* c, double s) {
  switch (c->loss) {
    case SCS_LOSS_LOGISTIC_MARGIN: return c->scale * s;
    case SCS_LOSS_LOGISTIC_CE: return -c->scale * s;
    case SCS_LOSS_LEAST_SQUARES: return 0.5 * s * c->scale;
    case SCS_LOSS_SOFTMAX_CE: return -c->scale * s;
    case SCS_LOSS_MULTI_LS: return 0.5 * s * c->scale;
    default: return s;
  }
}

// rocprofv3's name of the A x kernel on an fp32-stored dense A (scs_kernel_names)
const char* const GEMV_N_F32_NAME = "gemv_n_kernel<float>";

// z-partials of A x into c->zpart (dense: `nsplit` column splits; sparse: one
// CSR gather pass).  Returns the number of partials written.
int matvec_n(scs_ctx* c, const double* xd, int nsplit) {
  if (c->sparse && multi(c)) {   // Z = A X on the blocked CSR: part[(group*K + l)*Npad + n]
    const auto& B = c->bcsr;
    const int K = c->nout;
    if (B.kp > 1) {   // one pass over the nonzeros for all K columns (multi_sparse.hip)
      HCK(launch_multi_spmm_pack(xd, c->dc, c->dc, c->dcp, K, c->mXt, c->st));
      HCK(launch_multi_spmm(B.ptr, B.lidx, B.val, c->sp_f32, c->mXt, K, c->N, c->dc, B.shift, c->zpart, c->Npad,
                            c->st, B.narrow));
      c->prod_kname = multi_spmm_kernel_name(c->sp_f32, K, B.narrow);
    } else {          // the loop arm: column l of vec(X) is contiguous at x + d*l
      for (int l = 0; l < K; ++l)
        HCK(launch_spmv_blk(B.ptr, B.lidx, B.val, c->sp_f32, xd + c->dc * l, c->N, c->dc, B.shift, c->nnz,
                            c->zpart + (int64_t)l * c->Npad, (int64_t)K * c->Npad, c->st));
      c->prod_kname = spmv_kernel_name(c->sp_f32);
    }
    return blk_groups(B);
  }
  if (c->sparse) {
    const auto& B = c->bcsr;
    const int vk = c->sp_f32 ? (c->f32c ? 2 : 1) : 0;
    HCK(launch_spmv_blk(B.ptr, B.lidx, B.val, vk, xd, c->N, c->m, B.shift, c->nnz, c->zpart, c->Npad, c->st));
    c->prod_kname = spmv_kernel_name(vk);
    return B.nblk;
  }
  if (multi(c)) {   // Z = A X: x = vec(X) repacked K-contiguous, then one pass over A for all K columns
    HCK(launch_multi_pack_x(xd, c->dc, c->dcp, c->nout, c->mXt, c->st));
    HCK(launch_multi_ax(c->A, c->a32, c->nstage, c->Npad, c->dcp, c->nout, c->mXt, nsplit, c->zpart, c->st));
    return nsplit;
  }
  HCK(launch_gemv_n(c->A, c->a32, c->nstage, c->Npad, c->dcp, xd, nsplit, c->zpart, c->Npad, c->st));
  if (c->a32) c->prod_kname = GEMV_N_F32_NAME;
  return nsplit;
}

// the partial rows of Aᵀ v over the local rows into c->tpart (stride mpad); returns their count
int matvec_t_part(scs_ctx* c, const double* v) {
  if (c->sparse && multi(c))
    fail(c, SCS_ERR_ARG, "internal: the single-vector Aᵀv partials do not serve a multi-output context");
  if (c->sparse) {
    const auto& B = c->bcsc;
    const int vk = c->sp_f32 ? (c->f32c ? 2 : 1) : 0;
    HCK(launch_spmv_blk(B.ptr, B.lidx, B.val, vk, v, c->m, c->N, B.shift, c->nnz, c->tpart, c->mpad, c->st));
    return B.nblk;
  }
  if (multi(c)) fail(c, SCS_ERR_ARG, "internal: the single-vector Aᵀv partials do not serve a multi-output context");
  HCK(launch_gemv_t(c->A, c->a32, c->nstage, c->Npad, c->dc, c->dcp, v, c->tpart, c->st));
  return c->nchunk;
}

// the grow-only K-contiguous copy of an N x K operand (launch_multi_pack_v)
double* multi_vt(scs_ctx* c, int64_t need) {
  if (c->mVt_cap < need) {
    dfree_t(c, c->mVt);
    c->mVt_cap = 0;
    c->mVt = dalloc<double>(c, need);
    c->mVt_cap = need;
  }
  return c->mVt;
}

// out (device, m) = Aᵀ v over the local rows (dense: chunked column sums +
// fixed-order finalize; sparse: one CSC gather pass)
void matvec_t(scs_ctx* c, const double* v, double* out) {
  if (multi(c) && c->sparse) {   // vec(Aᵀ V) on the blocked CSC: part[(group*K + l)*dcp + j]
    const auto& B = c->bcsc;
    const int K = c->nout;
    if (B.kp > 1) {
      double* Vt = multi_vt(c, c->Npad * B.kp);
      HCK(launch_multi_spmm_pack(v, c->Npad, c->Npad, c->Npad, K, Vt, c->st));
      HCK(launch_multi_spmm(B.ptr, B.lidx, B.val, c->sp_f32, Vt, K, c->dc, c->N, B.shift, c->tpart, c->dcp, c->st,
                            B.narrow));
    } else {
      for (int l = 0; l < K; ++l)
        HCK(launch_spmv_blk(B.ptr, B.lidx, B.val, c->sp_f32, v + (int64_t)l * c->Npad, c->dc, c->N, B.shift, c->nnz,
                            c->tpart + (int64_t)l * c->dcp, (int64_t)K * c->dcp, c->st));
    }
    HCK(launch_multi_atv_finalize(c->tpart, blk_groups(B), K, c->dcp, c->dc, out, c->st));
    return;
  }
  if (multi(c)) {   // vec(Aᵀ V), V N x K (stride Npad): chunk partials of all K columns in one pass over A
    const int K = c->nout;
    double* Vt = multi_vt(c, c->Npad * K);
    HCK(launch_multi_pack_v(v, c->Npad, c->Npad, K, Vt, c->st));
    HCK(launch_multi_atv(c->A, c->a32, c->nstage, c->Npad, c->dc, c->dcp, K, Vt, c->tpart, c->st));
    HCK(launch_multi_atv_finalize(c->tpart, c->nchunk, K, c->dcp, c->dc, out, c->st));
    return;
  }
  const int np = matvec_t_part(c, v);
  HCK(launch_gemv_t_finalize(c->tpart, np, c->mpad, c->m, out, c->st));
}

void require_dense(scs_ctx* c, const char* what) {
  if (c->sparse)
    fail(c, SCS_ERR_ARG, "%s needs a dense A (sparse A supports f, ∇f and ProxLQNSCORE)", what);
  if (c->a32) fail(c, SCS_ERR_ARG, "%s needs an fp64-stored A: fp32 storage (scs_set_dense_f32) does not cover it", what);
}

// SCS_LOSS_SAMPLEWISE, host mode: the pinned copy of the current view's y (n entries), downloaded when
// the view (device pointer, rows, y_stamp) is not among the four held
const double* sw_host_y(scs_ctx* c) {
  const int64_t n = c->N;
  for (auto& e : c->swy)
    if (e.key == c->y && e.n == n && e.stamp == c->y_stamp) return e.h;
  auto& e = c->swy[c->swy_next];
  c->swy_next = (c->swy_next + 1) % 4;
  e.key = nullptr;
  if (e.cap < n) {
    if (e.h) HCK(hipHostFree(e.h));
    e.h = nullptr;
    e.cap = 0;
    HCK(hipHostMalloc((void**)&e.h, std::max<int64_t>(n, 1) * sizeof(double), hipHostMallocDefault));
    e.cap = std::max<int64_t>(n, 1);
  }
  if (n > 0) d2h(c, e.h, c->y, n);
  sync(c);
  e.key = c->y;
  e.n = n;
  e.stamp = c->y_stamp;
  return e.h;
}

// The loss epilogue of the current view: every launch_epilogue of the data path goes through here.
// zpart: `ns` z-partials (stride Npad); zout: where z goes with EPI_Z.  The menu kinds launch
// epilogue_kernel.  SCS_LOSS_SAMPLEWISE (1) materialises z (the EPI_Z pass of epilogue_kernel: into
// zout with EPI_Z, else into scratch -- a line-search trial or the held-out set must not overwrite the
// cached c->z; one partial without EPI_Z is z already), (2) asks the caller's functions for exactly
// what `flags` needs and (3) launches samplewise_epilogue_kernel over their output.
void loss_epilogue(scs_ctx* c, int flags, const double* zpart, int ns, double* zout) {
  if (multi(c)) {   // R -> gN, P -> hN (N x K, stride Npad), s_i = Σ_k Y_ik -> vN
    if (!multi_loss(c->loss)) fail(c, SCS_ERR_ARG, "a multi-output context (scs_set_outputs) takes SCS_LOSS_SOFTMAX_CE or "
                                                   "SCS_LOSS_MULTI_LS");
    HCK(launch_multi_epilogue(c->loss, flags, c->nout, zpart, ns, c->y, c->N, c->Npad, c->scale, zout, c->gN, c->hN,
                              c->vN, c->valpart, c->st));
    return;
  }
  if (c->loss != SCS_LOSS_SAMPLEWISE) {
    HCK(launch_epilogue(c->loss, c->ggn, flags, zpart, ns, c->Npad, c->y, c->N, c->Npad, c->scale, zout, c->gN, c->hN,
                        c->wN, c->vN, c->valpart, c->st));
    return;
  }
  const int need = flags & ~EPI_Z;
  if (!c->sw) fail(c, SCS_ERR_STATE, "no sample-wise loss functions: call scs_set_loss_samplewise");
  const int64_t N = c->N, Npad = c->Npad;
  if (need && c->sw_cap < Npad) {
    dfree_t(c, c->swd);
    c->sw_cap = 0;
    c->swd = dalloc<double>(c, 5 * (size_t)Npad);
    c->sw_cap = Npad;
  }
  const double* z = zpart;
  if ((flags & EPI_Z) || ns != 1) {
    double* zm = (flags & EPI_Z) ? zout : c->swd;
    if (zm != zpart || ns != 1)
      HCK(launch_epilogue(SCS_LOSS_LEAST_SQUARES, SCS_GGN_NONE, EPI_Z, zpart, ns, Npad, c->y, N, Npad, 1.0, zm, nullptr,
                          nullptr, nullptr, nullptr, c->valpart, c->st));
    z = zm;
  }
  if (!need) return;
  int what = 0;
  if (need & EPI_VAL) what |= SCS_SW_VALUE;
  if (need & EPI_GRAD) what |= SCS_SW_D1;
  if (need & EPI_HESS) what |= SCS_SW_D2;
  if (need & EPI_GGN) {
    if (need & (EPI_GRAD | EPI_HESS)) fail(c, SCS_ERR_ARG, "sample-wise loss: d1 / d2 carry r / q of the GGN request");
    if (!c->sw_ggn) fail(c, SCS_ERR_ARG, "ProxGGNSCORE needs an out_fn / GGN loss kind (scs_set_loss_samplewise "
                                         "without has_ggn)");
    what |= SCS_SW_GGN;
  }
  double *dv = c->swd + c->sw_cap, *d1 = dv + c->sw_cap, *d2 = d1 + c->sw_cap, *ds = d2 + c->sw_cap;
  int rc;
  if (c->sw_dev) {
    rc = N > 0 ? c->sw(c->sw_user, what, N, z, c->y, dv, d1, d2, ds, (void*)c->st) : 0;
  } else {
    if (c->swh_cap < N) {
      sync(c);   // uploads from the old buffer
      if (c->swh) HCK(hipHostFree(c->swh));
      c->swh = nullptr;
      c->swh_cap = 0;
      HCK(hipHostMalloc((void**)&c->swh, 5 * (size_t)N * sizeof(double), hipHostMallocDefault));
      c->swh_cap = N;
    }
    const int64_t hc = c->swh_cap;
    double *hz = c->swh, *hv = hz + hc, *h1 = hv + hc, *h2 = h1 + hc, *hs = h2 + hc;
    const double* hy = sw_host_y(c);
    // (the stream is in order: the previous call's uploads from these buffers precede this download)
    if (N > 0) d2h(c, hz, z, N);
    sync(c);
    rc = N > 0 ? c->sw(c->sw_user, what, N, hz, hy, hv, h1, h2, hs, nullptr) : 0;
    if (rc == 0 && N > 0) {
      if (what & SCS_SW_VALUE) h2d(c, dv, hv, N);
      if (what & (SCS_SW_D1 | SCS_SW_GGN)) h2d(c, d1, h1, N);
      if (what & (SCS_SW_D2 | SCS_SW_GGN)) h2d(c, d2, h2, N);
      if (what & SCS_SW_GGN) h2d(c, ds, hs, N);
    }
  }
  if (rc != 0) {
    invalidate_caches(c);   // z was replaced, its value was not
    fail(c, SCS_ERR_CALLBACK, "sample-wise loss callback (what = %d) returned %d", what, rc);
  }
  HCK(launch_samplewise_epilogue(need, dv, d1, d2, ds, N, Npad, c->gN, c->hN, c->wN, c->vN, c->valpart, c->st));
}

// Forward pass at the device vector xd whose host copy is xh: z = A x (or the
// cached z), then the epilogue with `flags`.  Always refreshes the f-value
// cache; returns f(x) (global).
double forward(scs_ctx* c, const double* xh, const double* xd, int flags, bool need_val = true) {
  const bool cached = c->zvalid && key_hit(c, c->zkey, c->ztag, xh);
  hipEvent_t e0;
  if (!cached) {
    tbegin(c, T_GEMV, &e0);
    const int ns = matvec_n(c, xd, c->nsplit);
    tend(c, T_GEMV, e0);
    flags |= EPI_Z | EPI_VAL;
    loss_epilogue(c, flags, c->zpart, ns, c->z);
    // loss sum -> scal[ZF_SLOT] (reduce buffer slot 0 in multi-rank); a slot of its own: the value
    // stays in flight until the next use (no host round trip when the caller only needs z)
    ensure_red(c);
    double* dst = sharded(c) ? c->red : c->scal + ZF_SLOT;
    HCK(launch_sum_partials(c->valpart, c->nval, dst, c->st));
    allreduce(c, c->red, 1);
    if (sharded(c)) HCK(hipMemcpyAsync(c->scal + ZF_SLOT, c->red, sizeof(double), hipMemcpyDeviceToDevice, c->st));
    d2h(c, c->hscal + ZF_SLOT, c->scal + ZF_SLOT, 1);
    c->zf_pending = true;
    key_set(c, c->zkey, c->ztag, xh);
    c->zvalid = true;
  } else if (flags & ~(EPI_VAL | EPI_Z)) {
    flags &= ~(EPI_Z | EPI_VAL);
    loss_epilogue(c, flags, c->z, 1, c->z);
  }
  if (need_val && c->zf_pending) {
    sync(c);
    c->zfval = loss_scale_value(c, c->hscal[ZF_SLOT]);
    c->zf_pending = false;
  }
  return c->zfval;
}

// out (device, m) = Aᵀ v over the local rows (no reduction)
void gemv_t_local(scs_ctx* c, const double* v, double* out) {
  hipEvent_t e0;
  tbegin(c, T_GEMV, &e0);
  matvec_t(c, v, out);
  tend(c, T_GEMV, e0);
}

// out (device, m) = Aᵀ v (local, then all-reduced across ranks)
void gemv_t_global(scs_ctx* c, const double* v, double* out) {
  hipEvent_t e0;
  tbegin(c, T_GEMV, &e0);
  ensure_red(c);
  matvec_t(c, v, sharded(c) ? c->red : out);
  tend(c, T_GEMV, e0);
  if (sharded(c)) {
    allreduce(c, c->red, c->m);
    HCK(hipMemcpyAsync(out, c->red, sizeof(double) * c->m, hipMemcpyDeviceToDevice, c->st));
  }
}

// SCS_LOSS_CALLBACK: call the caller's loss with x (the host copy xh, or xd downloaded) and
// return the host output area (nout doubles) of the pinned exchange buffer.  The stream is
// drained first: the previous upload from the buffer must have landed before it is reused.
double* cb_eval(scs_ctx* c, int what, const double* xh, const double* xd, size_t nout) {
  if (!c->cb) fail(c, SCS_ERR_STATE, "no loss callback: call scs_set_loss_callback");
  const int64_t m = c->m;
  const size_t need = (size_t)m + nout;
  sync(c);
  if (need > c->cbh_cap) {
    if (c->cbh) HCK(hipHostFree(c->cbh));
    c->cbh = nullptr;
    c->cbh_cap = 0;
    HCK(hipHostMalloc((void**)&c->cbh, need * sizeof(double), hipHostMallocDefault));
    c->cbh_cap = need;
  }
  double* xb = c->cbh;
  if (xh) {
    std::memcpy(xb, xh, sizeof(double) * m);
  } else {
    d2h(c, xb, xd, m);
    sync(c);
  }
  const int rc = c->cb(c->cb_user, what, xb, m, xb + m);
  if (rc == SCS_CB_NO_METHOD && what == SCS_CB_GRAD_X)   // prox-GGN-SCORE.jl:59 called grad_fx(x)
    fail(c, SCS_ERR_REF, "MethodError: no method matching grad_fx(::Vector{Float64}) (ProxGGNSCORE calls "
                         "model.grad_fx(x) with one argument in its ss_type 3 line search, "
                         "prox-GGN-SCORE.jl:58-59,83-84)");
  if (rc != 0) fail(c, SCS_ERR_CALLBACK, "loss callback (what = %d) returned %d", what, rc);
  return xb + m;
}

// f(x) for a device vector with host copy xh
double eval_f_dev(scs_ctx* c, const double* xh, const double* xd) {
  if (c->loss == SCS_LOSS_CALLBACK) return cb_eval(c, SCS_CB_F, xh, xd, 1)[0];
  if (c->loss == SCS_LOSS_ROSENBROCK) {
    HCK(launch_rosen(xd, c->m, 0, c->scal + 8, nullptr, 0, c->st));
    d2h(c, c->hscal + 8, c->scal + 8, 1);
    sync(c);
    return c->hscal[8];
  }
  if (c->loss == SCS_LOSS_QUADRATIC) {
    // 1/2*(x'*(A*x)) + y'*x
    require_dense(c, "the quadratic loss");
    HCK(launch_gemv_n(c->A, 0, c->nstage, c->Npad, c->mpad, xd, 1, c->zpart, c->Npad, c->st));
    HCK(launch_dot(xd, c->zpart, c->m, c->scal + 8, c->st));
    HCK(launch_dot(c->y, xd, c->m, c->scal + 9, c->st));
    d2h(c, c->hscal + 8, c->scal + 8, 2);
    sync(c);
    return 0.5 * c->hscal[8] + c->hscal[9];
  }
  return forward(c, xh, xd, 0);
}

// ftest(x) = f(Atest, ytest, x) (iterate.jl:173) at the device vector xd, enqueued: the loss sum of
// the held-out rows lands in scal[TF_SLOT] (all-reduced across ranks for a row-sharded test set);
// loss_scale_value(hscal / hloop[TF_SLOT]) is the value.  The same products and epilogue as f(x),
// on the held-out view; the z / f caches of the data are not touched.
void ftest_enqueue(scs_ctx* c, const double* xd) {
  ensure_red(c);   // sized by the data's view, before the held-out one is swapped in
  TestScope ts(c);
  const int ns = matvec_n(c, xd, c->nsplit);
  loss_epilogue(c, EPI_VAL, c->zpart, ns, c->z);
  double* dst = sharded(c) ? c->red : c->scal + TF_SLOT;
  HCK(launch_sum_partials(c->valpart, c->nval, dst, c->st));
  allreduce(c, c->red, 1);
  if (sharded(c)) HCK(hipMemcpyAsync(c->scal + TF_SLOT, c->red, sizeof(double), hipMemcpyDeviceToDevice, c->st));
}

// ftest(x) now (host copy xh, may be null, and device copy xd)
double eval_ftest_dev(scs_ctx* c, const double* xh, const double* xd) {
  if (!c->tset.on) fail(c, SCS_ERR_STATE, "no test data: call scs_set_test_data first");
  if (c->tset.host) return cb_eval(c, SCS_CB_FTEST, xh, xd, 1)[0];
  if (c->loss == SCS_LOSS_QUADRATIC) {   // 1/2*(x'*(Atest*x)) + ytest'*x
    // Atest*x and x' need Atest to be m x m (and ytest length m); Julia raises DimensionMismatch.
    // The test view holds only its own rows, so a non-square Atest must not reach eval_f_dev
    if (c->tset.v.Nglob != c->m)
      fail(c, SCS_ERR_ARG, "DimensionMismatch: the quadratic loss 1/2*(x'*(Atest*x)) + ytest'*x needs an m x m "
                           "Atest (m = %lld), got %lld rows", (long long)c->m, (long long)c->tset.v.Nglob);
    TestScope ts(c);
    return eval_f_dev(c, xh, xd);
  }
  ftest_enqueue(c, xd);
  d2h(c, c->hscal + TF_SLOT, c->scal + TF_SLOT, 1);
  sync(c);
  return loss_scale_value(c, c->hscal[TF_SLOT]);
}

// ∇f(x) -> out (device)
// (cb_what: SCS_CB_GRAD = grad_fx(A, y, x); SCS_CB_GRAD_X = ProxGGNSCORE's one-argument call)
void grad_f_dev(scs_ctx* c, const double* xh, const double* xd, double* out, int cb_what = SCS_CB_GRAD) {
  if (c->gfix) {   // step!(...; ∇fx): grad_f = x -> ∇fx at every point (prox-L-BFGS-SCORE.jl:98-100)
    if (out != c->gfix) HCK(hipMemcpyAsync(out, c->gfix, sizeof(double) * c->m, hipMemcpyDeviceToDevice, c->st));
    return;
  }
  if (c->loss == SCS_LOSS_CALLBACK) {
    const double* g = cb_eval(c, cb_what, xh, xd, c->m);
    HCK(hipMemcpyAsync(out, g, sizeof(double) * c->m, hipMemcpyHostToDevice, c->st));
    return;
  }
  if (c->loss == SCS_LOSS_ROSENBROCK) {
    HCK(launch_rosen(xd, c->m, 1, out, nullptr, 0, c->st));
    return;
  }
  if (c->loss == SCS_LOSS_QUADRATIC) {
    // 0.5*(A*x + Aᵀ*x) + y
    require_dense(c, "the quadratic loss");
    HCK(launch_gemv_n(c->A, 0, c->nstage, c->Npad, c->mpad, xd, 1, c->zpart, c->Npad, c->st));
    gemv_t_global(c, xd, c->gtmp2);
    HCK(launch_axpby(c->zpart, 1.0, c->gtmp2, c->m, c->gtmp2, c->st));
    HCK(launch_axpby(c->y, 0.5, c->gtmp2, c->m, out, c->st));  // y + 0.5*(Ax + Aᵀx)
    return;
  }
  forward(c, xh, xd, EPI_GRAD, false);
  gemv_t_global(c, c->gN, out);
}

// ∇q(x) = ∇f(x) + λ hμ.grad(x) -> out (device); uses the 2-slot cache.
void grad_q_dev(scs_ctx* c, const double* xh, const double* xd, double* out, int cb_what = SCS_CB_GRAD) {
  // (a one-argument grad_fx call is always made: a cached grad_fx(A, y, x) must not stand in for it)
  const bool cacheable = !(c->loss == SCS_LOSS_CALLBACK && cb_what == SCS_CB_GRAD_X);
  for (int s = 0; s < 2 && cacheable; ++s)
    if (c->gvalid[s] && key_hit(c, c->gkey[s], c->gtag[s], xh)) {
      HCK(hipMemcpyAsync(out, c->gcache[s], sizeof(double) * c->m, hipMemcpyDeviceToDevice, c->st));
      return;
    }
  grad_f_dev(c, xh, xd, c->gtmp, cb_what);
  HCK(launch_smoother(c->smooth, xd, c->m, c->mu, c->slb, c->sub, c->wel, c->zb, c->hinv, c->st));
  HCK(launch_axpby(c->gtmp, c->lam, c->zb, c->m, out, c->st));
  if (!cacheable) return;
  const int s = c->gnext;
  c->gnext ^= 1;
  HCK(hipMemcpyAsync(c->gcache[s], out, sizeof(double) * c->m, hipMemcpyDeviceToDevice, c->st));
  key_set(c, c->gkey[s], c->gtag[s], xh);
  c->gvalid[s] = true;
}

double eval_reg_dev(scs_ctx* c, const double* xd) {
  HCK(launch_reg_value(prox_args(c), xd, c->m, c->scal + 10, c->scal + 64 + 2 * 256, c->st));
  d2h(c, c->hscal + 10, c->scal + 10, 1);
  sync(c);
  return c->hscal[10];
}

// linesearch (utils.jl:27-35): Armijo with ρ = 0.5, c = 1e-4 and no cap.
// obj(x) and grad_q(x) are evaluated once (the reference re-evaluates the
// same deterministic values on every trial).  For the data losses the trial's
// f(x + αd) is formed incrementally: A(x + αd) = Ax + α·Ad with
// Ax from f(x)'s forward pass and ONE extra pass for Ad, then O(N) per trial (the
// epilogue over z0 + α·zd) instead of a full pass over A per trial.  The values
// equal the direct form to rounding (SCS_LS_INCR=0 keeps the direct form).
bool ls_incremental(const scs_ctx* c) {
  const char* e = std::getenv("SCS_LS_INCR");   // read per call (A/B within one process)
  const bool off = e && e[0] == '0';
  return !off && !c->generic && (c->loss == SCS_LOSS_LOGISTIC_MARGIN || c->loss == SCS_LOSS_LOGISTIC_CE ||
                                 c->loss == SCS_LOSS_LEAST_SQUARES || c->loss == SCS_LOSS_SAMPLEWISE ||
                                 multi_loss(c->loss));
}

double line_search(scs_ctx* c, const double* xh, const double* xd, const double* dd) {
  const double f0 = eval_f_dev(c, xh, xd) + eval_reg_dev(c, xd);
  // ProxGGNSCORE's grad_f is x -> model.grad_fx(x), one argument (prox-GGN-SCORE.jl:58-59,83-84):
  // a callback loss is asked for that call (a data problem's grad_fx(A, y, x) raises MethodError)
  grad_q_dev(c, xh, xd, c->gqn, c->method == SCS_PROX_GGNSCORE ? SCS_CB_GRAD_X : SCS_CB_GRAD);
  HCK(launch_dot(c->gqn, dd, c->m, c->scal + 11, c->st));
  d2h(c, c->hscal + 11, c->scal + 11, 1);
  sync(c);
  const double gd = c->hscal[11];
  const bool incr = ls_incremental(c);
  double* zd = nullptr;
  double* pair = nullptr;
  if (incr) {
    // z0 = A x: f(x) above left it in c->z (forward with EPI_Z); A d once into zd
    forward(c, xh, xd, 0);
    const int64_t nz = c->Npad * kout(c);   // a multi-output z is N x K: the pair is two slices of K columns
    if (c->lscap < 3 * nz) {
      dfree_t(c, c->lsbuf);
      c->lsbuf = dalloc<double>(c, 3 * nz);
      c->lscap = 3 * nz;
    }
    pair = c->lsbuf;
    zd = c->lsbuf + 2 * nz;
    hipEvent_t e0;
    tbegin(c, T_GEMV, &e0);
    const int ns = matvec_n(c, dd, c->nsplit);
    tend(c, T_GEMV, e0);
    loss_epilogue(c, EPI_Z, c->zpart, ns, zd);
    ensure_red(c);
  }
  // the band (relative) within which an incremental trial is re-decided on the direct form;
  // SCS_LS_NEAR overrides it (tests: a huge band re-decides every trial).  The incremental form's own
  // rounding is one extra addition per z_i (<= eps·(|Ax|_i + α|Ad|_i)): ~1e-16 relative in f; both
  // forms share the dot products' rounding.  1e-12 leaves four orders of margin (the first r05
  // value, 1e-9, re-decided trials whose margin was a million times the incremental form's rounding)
  const char* ne = std::getenv("SCS_LS_NEAR");
  const double near = ne ? std::atof(ne) : 1e-12;
  double alpha = 1.0;
  for (int trial = 0; trial < 100000; ++trial) {
    // the trial point lives on the device only (no host copy: it is keyed by a fresh tag)
    HCK(launch_trial_point(xd, dd, alpha, c->m, c->gtmp2, c->st));
    double ft;
    if (incr) {
      HCK(launch_ls_pair(c->z, zd, alpha, c->Npad * kout(c), pair, c->st));
      loss_epilogue(c, EPI_VAL, pair, 2, nullptr);   // (a sample-wise trial's z goes to scratch, not over c->z)
      double* dst = sharded(c) ? c->red : c->scal + 14;
      HCK(launch_sum_partials(c->valpart, c->nval, dst, c->st));
      allreduce(c, c->red, 1);
      if (sharded(c)) HCK(hipMemcpyAsync(c->scal + 14, c->red, sizeof(double), hipMemcpyDeviceToDevice, c->st));
      d2h(c, c->hscal + 14, c->scal + 14, 1);
      const double rg = eval_reg_dev(c, c->gtmp2);   // syncs: hscal[14] has landed too
      ft = loss_scale_value(c, c->hscal[14]) + rg;
      // Ax + fl(α·Ad) differs from the reference's A·fl(x + αd) (utils.jl:27-35) in the last bits
      // of each z_i: a trial whose Armijo test sits within `near` (relative) of its threshold is
      // decided on the direct form instead, so the accepted α is the reference's form's
      if (std::fabs(ft - (f0 + 1e-4 * alpha * gd)) <= near * std::max(std::fabs(f0), std::fabs(ft))) {
        ft = eval_f_dev(c, nullptr, c->gtmp2) + eval_reg_dev(c, c->gtmp2);
        ++c->ls_direct;
        // that pass left A·(x + αd) in c->z: restore z0 = A x for the later incremental trials
        if (ft > f0 + 1e-4 * alpha * gd) forward(c, xh, xd, 0, false);
      }
    } else {
      ft = eval_f_dev(c, nullptr, c->gtmp2) + eval_reg_dev(c, c->gtmp2);
    }
    if (!(ft > f0 + 1e-4 * alpha * gd)) return alpha;
    alpha = 0.5 * alpha;
  }
  fail(c, SCS_ERR_REF, "linesearch did not terminate");
}

// solve (G + λ diag Hr) sol = rhs in place (rhs -> sol, length m_pad, zero-padded).
// Hand-written blocked Cholesky on MFMA (chol.hip) first; the hand-written blocked LU with
// partial pivoting (lu.hip; the reference's `\`, prox-N-SCORE.jl:70) from the saved copy when
// a pivot is not positive (e.g. the indefinite Q of a CE loss on ±1 labels,
// test/test_algs.jl:10), or always with force_lu (scs_solve_eval).
// SCS_FAULT_LATE (tests; read per call): a bit mask of the dependency waits to report as timed out,
// as the device would after ~30 s (never expected), so that each fallback below can be driven:
// 1 the one-launch triangular solves, 2 the QR's one-launch backward solve, 4 the dependency-driven
// Cholesky chain (SCS_CHOL_DAG=1), 8 the pipelined factor's strip wait (SCS_CHOL_PIPE).  The
// cooperative LU panel's own give-up path is driven on the device instead (SCS_LU_COOP_SPIN=0).
static bool fault_late(int bit) {
  const char* e = std::getenv("SCS_FAULT_LATE");
  return e && (std::atoi(e) & bit);
}

// lu_factor(M) with the cooperative panel's fallback (r06).  A panel launch the runtime refuses runs as
// column steps inside lu_factor; a candidate exchange that timed out (info = -1: a workgroup of the
// one-launch panel never became resident -- the plain launch mode, SCS_LU_COOP_LAUNCH=0, or a device
// shared with other work) leaves M undefined, so `rebuild` restores the system and the factorization
// is redone with the column-step panels, which give the same factor and pivots bit for bit
// (test_lu_coop_panel_largest_grid).  Returns the factorization's info (0, or the first zero pivot).
template <class F>
int lu_factor_checked(scs_ctx* c, double* M, int64_t ld, int64_t n, int64_t npad, int* dinfo, F&& rebuild) {
  int info = 0;
  const int64_t refused0 = c->lu.coop_refused;
  HCK(hipMemsetAsync(dinfo, 0, sizeof(int), c->st));
  HCK(lu_factor(M, ld, n, npad, &c->lu, dinfo, c->st));
  HCK(hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, c->st));
  sync(c);
  c->fb[SCS_FB_LU_COOP_REFUSED] += c->lu.coop_refused - refused0;
  if (info != -1) return info;
  ++c->fb[SCS_FB_LU_COOP_REDO];
  rebuild();
  c->lu.no_coop = true;
  HCK(hipMemsetAsync(dinfo, 0, sizeof(int), c->st));
  const hipError_t e = lu_factor(M, ld, n, npad, &c->lu, dinfo, c->st);
  c->lu.no_coop = false;
  HCK(e);
  HCK(hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, c->st));
  sync(c);
  if (info < 0) fail(c, SCS_ERR_HIP, "LU: info %d from the column-step panels", info);
  return info;
}

// chol_solve with the one-launch solves' fallback (r06): a dependency wait of chol_fwd/bwd_persist_kernel
// that gave up (~30 s, never expected: a block waits only on blocks dispatched before it) sets caux.serr
// and leaves rhs undefined; the solve is redone from the saved right-hand side by the per-block launches
// (SCS_SOLVE_PERSIST=0's form)
// (CholSys: the buffers one Cholesky solve works on -- a step's own, step_chol, or scs_chol_eval's)
struct CholSys {
  double* G;             // the upper system, column-major ld x ld, factored in place
  int64_t m, ld;         // order and padded order
  double* W;             // [ld/128][128*128] inverted diagonal blocks
  CholAux* aux;
  const int2* trilist;   // row-major lower tiles of ld/128 blocks
  double* ysol;          // (ld) triangular-solve scratch
  double* rbk;           // (ld) the right-hand side before a one-launch solve
  int* info;             // device info word
};
static CholSys step_chol(scs_ctx* c) {
  return {c->G, c->m, c->mpad, c->W, &c->caux, c->trilist, c->ysol, c->rbk, c->cinfo};
}

void chol_solve_checked(scs_ctx* c, const CholSys& s, double* rhs) {
  const int64_t ld = s.ld;
  HCK(hipMemcpyAsync(s.rbk, rhs, sizeof(double) * ld, hipMemcpyDeviceToDevice, c->st));
  HCK(chol_solve(s.G, ld, ld, s.W, rhs, s.ysol, s.aux, c->st));
  int late = 0;
  if (s.aux->serr) HCK(hipMemcpyAsync(&late, s.aux->serr, sizeof(int), hipMemcpyDeviceToHost, c->st));
  sync(c);
  if (!late && !fault_late(1)) return;
  if (s.aux->serr) HCK(hipMemsetAsync(s.aux->serr, 0, sizeof(int), c->st));
  ++c->fb[SCS_FB_SOLVE_BLOCKS];
  HCK(hipMemcpyAsync(rhs, s.rbk, sizeof(double) * ld, hipMemcpyDeviceToDevice, c->st));
  s.aux->no_persist = true;
  const hipError_t e = chol_solve(s.G, ld, ld, s.W, rhs, s.ysol, s.aux, c->st);
  s.aux->no_persist = false;
  HCK(e);
}

// chol_factor(s.G) with the chain launches' fallback: a dependency wait that gave up (~30 s: never
// expected) leaves the factor incomplete, so `restore` puts the system back and the factor is redone
// with one launch per operation (r06; was SCS_ERR_HIP).  Returns the factorization's info (0, or the
// first non-positive pivot, 1-based).
template <class F>
int chol_factor_checked(scs_ctx* c, const CholSys& s, F&& restore) {
  int info = 0;
  HCK(hipMemsetAsync(s.info, 0, sizeof(int), c->st));
  s.aux->chain_mode = c->rccl ? 2 : 0;   // RCCL's streams in the process: keep the factor's two apart
  HCK(chol_factor(s.G, s.ld, s.m, s.ld, s.W, s.aux, s.trilist, s.info, c->st));
  HCK(hipMemcpyAsync(&info, s.info, sizeof(int), hipMemcpyDeviceToHost, c->st));
  int late = 0;   // a dependency wait of the chain launches gave up (~30 s): never expected
  HCK(hipMemcpyAsync(&late, s.aux->serr, sizeof(int), hipMemcpyDeviceToHost, c->st));
  sync(c);
  if (late || (fault_late(4) && chol_dag_active(s.aux))) {
    HCK(hipMemsetAsync(s.aux->serr, 0, sizeof(int), c->st));
    ++c->fb[SCS_FB_CHAIN_REDO];
    restore();
    HCK(hipMemsetAsync(s.info, 0, sizeof(int), c->st));
    s.aux->no_dag = true;
    const hipError_t e = chol_factor(s.G, s.ld, s.m, s.ld, s.W, s.aux, s.trilist, s.info, c->st);
    s.aux->no_dag = false;
    HCK(e);
    HCK(hipMemcpyAsync(&info, s.info, sizeof(int), hipMemcpyDeviceToHost, c->st));
    sync(c);
  }
  return info;
}

// the LU fallback: the full symmetric system from the copy Gc (rebuilt from the cached Gram when
// this step's Gram came from the cache), the reference's `\` (prox-N-SCORE.jl:70)
void solve_lu_fallback(scs_ctx* c, double* rhs, hipEvent_t e0) {
  const int64_t m = c->m, ld = c->mpad;
  int info = 0;
  if (c->g_from_cache) {
    HCK(hipMemcpyAsync(c->Gc, c->Gk, sizeof(double) * ld * ld, hipMemcpyDeviceToDevice, c->st));
    HCK(launch_diag_add(c->Gc, c->mpad, m, c->lam, c->Hr, c->st));
  }
  // the full symmetric matrix: its column-major storage is also the row-major one lu.hip factors
  HCK(launch_symmetrize(c->Gc, ld, m, c->st));
  // a NaN / Inf in the system (a smoother's NaN, Appendix A) is no SingularException in the
  // reference: LAPACK getrf only flags exact zero pivots, and the solve comes out NaN
  HCK(hipMemsetAsync(c->cinfo, 0, sizeof(int), c->st));
  HCK(launch_nonfinite(c->Gc, ld, m, rhs, c->cinfo, c->st));
  HCK(hipMemcpyAsync(&info, c->cinfo, sizeof(int), hipMemcpyDeviceToHost, c->st));
  sync(c);
  c->lu_fallback_used = true;
  if (info != 0) {
    HCK(launch_fill(rhs, m, std::numeric_limits<double>::quiet_NaN(), c->st));
    tend(c, T_SOLVE, e0);
    return;
  }
  HCK(lu_aux_init(&c->lu, ld, c->st));
  // the system the factor overwrites, kept for a column-step redo (lu_factor_checked)
  if (c->Gbk_n != ld) {
    dfree_t(c, c->Gbk);
    c->Gbk = dalloc<double>(c, (size_t)ld * ld);
    c->Gbk_n = ld;
  }
  HCK(hipMemcpyAsync(c->Gbk, c->Gc, sizeof(double) * ld * ld, hipMemcpyDeviceToDevice, c->st));
  info = lu_factor_checked(c, c->Gc, ld, m, ld, c->cinfo, [&] {
    HCK(hipMemcpyAsync(c->Gc, c->Gbk, sizeof(double) * ld * ld, hipMemcpyDeviceToDevice, c->st));
  });
  if (info != 0) fail(c, SCS_ERR_SOLVE, "SingularException(%d)", info);
  HCK(lu_solve(c->Gc, ld, ld, &c->lu, rhs, c->st));
  tend(c, T_SOLVE, e0);
}

// solve (G + λ diag Hr) sol = rhs in place (rhs -> sol, length m_pad, zero-padded).
// Hand-written blocked Cholesky on MFMA (chol.hip) first; the hand-written blocked LU with
// partial pivoting (lu.hip; the reference's `\`, prox-N-SCORE.jl:70) from the saved copy when
// a pivot is not positive (e.g. the indefinite Q of a CE loss on ±1 labels,
// test/test_algs.jl:10), or always with force_lu (scs_solve_eval).
// the reference's own solver (scs_set_solver(SCS_SOLVER_REFERENCE)): qr(JQJ) \ Je by Householder QR
// (prox-GGN-SCORE.jl:131) on the symmetrized copy Gc; a NaN / Inf system gives a NaN direction
// Householder QR solve of the column-major npad x npad system A (identity-padded) with b := A \ b;
// a backward-solve dependency wait that gave up (~30 s, never expected) fails the call
// r06: the panels as cooperative launches (qr.hip qr_panel_coop_kernel) -- a refused launch runs that panel
// by column steps inside qr_solve; a sweep that gave up (cinfo = -1: a workgroup never became resident)
// leaves A and b undefined, so the solve is redone from the saved copy with the per-column launches
// (q, bk, bk_n: the workspace and the redo copy -- a step's own, c->qr and c->qbk, or scs_qr_eval's)
static void qr_run(scs_ctx* c, QRAux* q, double*& bk, int64_t& bk_n, double* A, int64_t npad, double* b) {
  const bool coop = qr_coop_wanted(npad);
  const size_t nA = (size_t)npad * npad;
  if (coop) {
    if (bk_n != npad) {
      dfree_t(c, bk);
      bk = dalloc<double>(c, nA + (size_t)npad);
      bk_n = npad;
    }
    HCK(hipMemcpyAsync(bk, A, sizeof(double) * nA, hipMemcpyDeviceToDevice, c->st));
    HCK(hipMemcpyAsync(bk + nA, b, sizeof(double) * npad, hipMemcpyDeviceToDevice, c->st));
  }
  const int64_t refused0 = q->coop_refused;
  HCK(qr_solve(A, npad, npad, q, b, c->st));
  int late = 0, cinfo = 0;
  HCK(hipMemcpyAsync(&late, q->err, sizeof(int), hipMemcpyDeviceToHost, c->st));
  if (coop) HCK(hipMemcpyAsync(&cinfo, q->cinfo, sizeof(int), hipMemcpyDeviceToHost, c->st));
  sync(c);
  c->fb[SCS_FB_QR_COOP_REFUSED] += q->coop_refused - refused0;
  if (cinfo == -1) {
    ++c->fb[SCS_FB_QR_COOP_REDO];
    HCK(hipMemcpyAsync(A, bk, sizeof(double) * nA, hipMemcpyDeviceToDevice, c->st));
    HCK(hipMemcpyAsync(b, bk + nA, sizeof(double) * npad, hipMemcpyDeviceToDevice, c->st));
    q->no_coop = true;
    const hipError_t e = qr_solve(A, npad, npad, q, b, c->st);
    q->no_coop = false;
    HCK(e);
    HCK(hipMemcpyAsync(&late, q->err, sizeof(int), hipMemcpyDeviceToHost, c->st));
    sync(c);
  }
  if (late || fault_late(2)) {
    // R is complete and qr.Ym still holds Qᵀb (the one-launch kernel only reads it): the backward
    // solve again by the per-block launches
    HCK(hipMemsetAsync(q->err, 0, sizeof(int), c->st));
    ++c->fb[SCS_FB_QR_BLOCKS];
    HCK(chol_back_blocks(A, npad, npad, q->W, q->Ym, b, c->st));
  }
}

void solve_qr(scs_ctx* c, double* rhs, hipEvent_t e0) {
  const int64_t m = c->m, ld = c->mpad;
  if (c->g_from_cache) {
    HCK(hipMemcpyAsync(c->Gc, c->Gk, sizeof(double) * ld * ld, hipMemcpyDeviceToDevice, c->st));
    HCK(launch_diag_add(c->Gc, c->mpad, m, c->lam, c->Hr, c->st));
  }
  HCK(launch_symmetrize(c->Gc, ld, m, c->st));
  int info = 0;
  HCK(hipMemsetAsync(c->cinfo, 0, sizeof(int), c->st));
  HCK(launch_nonfinite(c->Gc, ld, m, rhs, c->cinfo, c->st));
  HCK(hipMemcpyAsync(&info, c->cinfo, sizeof(int), hipMemcpyDeviceToHost, c->st));
  sync(c);
  c->lu_fallback_used = false;
  if (info != 0) {
    HCK(launch_fill(rhs, m, std::numeric_limits<double>::quiet_NaN(), c->st));
    tend(c, T_SOLVE, e0);
    return;
  }
  HCK(qr_prepare(c->Gc, ld, m, ld, c->st));
  qr_run(c, &c->qr, c->qbk, c->qbk_n, c->Gc, ld, rhs);
  tend(c, T_SOLVE, e0);
}

void solve_system(scs_ctx* c, double* rhs, bool force_lu = false, bool force_qr = false) {
  const int64_t m = c->m, ld = c->mpad;
  hipEvent_t e0;
  tbegin(c, T_SOLVE, &e0);
  // the LU fallback needs the system the in-place factor destroys: copied up front, or -- when
  // this step's Gram came from the cache -- rebuilt from it only if the factor fails
  if (!c->g_from_cache) HCK(hipMemcpyAsync(c->Gc, c->G, sizeof(double) * ld * ld, hipMemcpyDeviceToDevice, c->st));
  if (c->solver == SCS_SOLVER_REFERENCE && !force_lu && !force_qr) {
    if (c->method == SCS_PROX_GGNSCORE) force_qr = true;   // qr(JQJ) \ Je
    else force_lu = true;                                  // (H + λHr) \ ∇q: Julia's `\` = LU
  }
  if (force_qr) {
    solve_qr(c, rhs, e0);
    return;
  }
  int info = 0;
  if (!force_lu) {
    const CholSys s = step_chol(c);
    // a redo's system: Gc, or the cached Gram + λ diag Hr
    info = chol_factor_checked(c, s, [&] {
      if (c->g_from_cache) {
        HCK(hipMemcpyAsync(c->G, c->Gk, sizeof(double) * ld * ld, hipMemcpyDeviceToDevice, c->st));
        HCK(launch_diag_add(c->G, c->mpad, m, c->lam, c->Hr, c->st));
      } else {
        HCK(hipMemcpyAsync(c->G, c->Gc, sizeof(double) * ld * ld, hipMemcpyDeviceToDevice, c->st));
      }
    });
    if (info == 0) {
      chol_solve_checked(c, s, rhs);
      solve_flag_copy(c);
      c->lu_fallback_used = false;
      tend(c, T_SOLVE, e0);
      return;
    }
  }
  solve_lu_fallback(c, rhs, e0);
}

// the pipelined path's solve: the factor (and Gc) are already enqueued (gram_factor_pipelined,
// which opened the T_SOLVE interval at the end of the Gram).  false: a strip wait gave up (~30 s,
// never expected) and the strip was factored incomplete -- the caller redoes the Gram, the factor
// and the solve without the pipeline (r06; was SCS_ERR_STATE)
bool solve_factored(scs_ctx* c, double* rhs, hipEvent_t e0) {
  int info = 0, late = 0;
  HCK(hipMemcpyAsync(&info, c->cinfo, sizeof(int), hipMemcpyDeviceToHost, c->st));
  if (c->gp_flag) HCK(hipMemcpyAsync(&late, c->gp_flag, sizeof(int), hipMemcpyDeviceToHost, c->st));
  sync(c);
  if (late || fault_late(8)) {
    if (c->gp_flag) HCK(hipMemsetAsync(c->gp_flag, 0, sizeof(int), c->st));
    ++c->fb[SCS_FB_PIPE_REDO];
    tend(c, T_SOLVE, e0);
    return false;
  }
  if (info == 0) {
    chol_solve_checked(c, step_chol(c), rhs);
    solve_flag_copy(c);
    c->lu_fallback_used = false;
    tend(c, T_SOLVE, e0);
    return true;
  }
  solve_lu_fallback(c, rhs, e0);
  return true;
}

// the main Gram launch (scheduled when gram_schedule built a work list)
// the panel-blocked A the Gram kernels read: A itself, or for a sparse A its dense mirror, built
// once (Jt*Q*Jt' of a SparseMatrixCSC, prox-GGN-SCORE.jl:129 / hess_fx, prox-N-SCORE.jl:55; the
// products Ax, Aᵀv keep running on the sparse copies)
// (dense_a32: what that block holds -- the mirror of a sparse A is always fp64)
int dense_a32(const scs_ctx* c) { return c->sparse ? 0 : c->a32; }
const double* dense_A(scs_ctx* c) {
  if (!c->sparse) return c->A;
  if (c->Ad) return c->Ad;
  const size_t bytes = (size_t)c->Npad * c->dcp * sizeof(double);   // the data view's columns
  size_t fr = 0, tot = 0;
  HCK(hipMemGetInfo(&fr, &tot));
  if (bytes + (size_t)c->mpad * c->mpad * 16 > fr)
    fail(c, SCS_ERR_ARG,
         "the GGN sample-space branch on a sparse A forms Aᵀ from a dense mirror of A (%.1f GiB) plus the "
         "m x m system; the device has %.1f GiB free",
         bytes / 1073741824.0, fr / 1073741824.0);
  c->Ad = dalloc<double>(c, bytes / sizeof(double));
  HCK(hipMemsetAsync(c->Ad, 0, bytes, c->st));
  HCK(launch_densify(c->rowptr, c->colidx, c->val, c->sp_f32, c->N, c->Npad, c->Ad, c->st));
  return c->Ad;
}

// The Gram of a sparse A priced by nnz (sparse_gram_kernel: Σ_r nnz_r² multiply-adds) instead of
// dense MFMA tiles over a densified A (N·m² whatever the density): chosen when Σ_r nnz_r² is below
// N·m²/64 (the dense tiles run ~50x more flops per second), or forced by SCS_SPARSE_GRAM=1 / 0.
// The sparse Gram's row copy: the (sorted) CSR cut into 2^sparse_gram_shift()-wide column blocks,
// unpadded (blk_count / blk_scan / blk_scatter with no slot rounding).
void build_gram_blocked(scs_ctx* c) {
  SpBlkT& B = c->bgram;
  const int64_t nrows = c->N;
  B.shift = sparse_gram_shift();
  B.nblk = (int)ceil_div(c->dc, int64_t(1) << B.shift);
  const int64_t nk = (int64_t)B.nblk * nrows;
  int64_t* cnt = dalloc<int64_t>(c, nk + 1);
  int64_t* first = dalloc<int64_t>(c, nk + 1);
  B.ptr = dalloc<int64_t>(c, nk + 1);
  int64_t nnz = 0;
  if (nrows > 0) {
    HCK(blk_count(c->rowptr, c->colidx, nrows, B.shift, cnt, first, c->st));
    size_t tb = 0;
    HCK(blk_scan(nullptr, &tb, cnt, B.ptr, nk + 1, c->st));
    void* tmp = dalloc<char>(c, tb);
    HCK(blk_scan(tmp, &tb, cnt, B.ptr, nk + 1, c->st));
    HCK(hipMemcpyAsync(&nnz, B.ptr + nk, sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
    sync(c);
    dfree(c, tmp);
  }
  B.nnz = nnz;
  B.lidx = dalloc<uint16_t>(c, nnz + 8);
  B.val = c->sp_f32 ? (void*)dalloc<float>(c, (size_t)nnz + 8) : (void*)dalloc<double>(c, (size_t)nnz + 8);
  if (nrows > 0)
    HCK(blk_scatter(c->rowptr, c->colidx, c->val, c->sp_f32, nrows, B.shift, B.ptr, first, B.lidx, B.val, c->st));
  sync(c);
  dfree_t(c, cnt);
  dfree_t(c, first);
}

// The variant-8 structure (sparse.hip, r04): the segment records, the per-triple table and the sw
// buffer.  Built only when it fits (free memory less 4 GiB) and its units fit 32 bits; else state -1
// and gram_sparse takes the Gram-blocked walk (variant 6).  C5 shape: T 47 GB, seg 6.9 GB, sw 5.5 GB.
bool build_gram_seg(scs_ctx* c) {
  scs_ctx::SegGram& S = c->sgseg;
  if (S.state) return S.state > 0;
  S.state = -1;
  const int64_t nrows = c->N, m = c->dc;   // the data view's columns
  const int shift = sparse_gram_shift();
  const int64_t nblk = ceil_div(m, int64_t(1) << shift);
  const int64_t nk = nblk * nrows;
  std::vector<int64_t> cp((size_t)m + 1), tp((size_t)m + 1, 0);
  HCK(hipMemcpyAsync(cp.data(), c->colptr, sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost, c->st));
  sync(c);
  for (int64_t j = 0; j < m; ++j) tp[(size_t)j + 1] = tp[(size_t)j] + ((j >> shift) + 1) * (cp[(size_t)j + 1] - cp[(size_t)j]);
  const int64_t nT = tp[(size_t)m], nnz = cp[(size_t)m];
  const double units_max = (double)seg_units_host(1, c->sp_f32) * (double)nnz + 2.0 * (double)nk;
  const double need = 8.0 * ((double)nT + (double)nnz + units_max + 4.0 * (double)(nk + 1)) + 4.0 * 1073741824.0;
  size_t fr = 0, tot = 0;
  HCK(hipMemGetInfo(&fr, &tot));
  if (nrows <= 0 || need > (double)fr) return false;
  int64_t* cnt = dalloc<int64_t>(c, nk + 1);
  int64_t* first = dalloc<int64_t>(c, nk + 1);
  int64_t* ucnt = dalloc<int64_t>(c, nk + 1);
  int64_t* uptr = dalloc<int64_t>(c, nk + 1);
  HCK(blk_count(c->rowptr, c->colidx, nrows, shift, cnt, first, c->st));
  HCK(seg_units(cnt, nk, c->sp_f32, ucnt, c->st));
  size_t tb = 0;
  HCK(blk_scan(nullptr, &tb, ucnt, uptr, nk + 1, c->st));
  void* tmp = dalloc<char>(c, tb);
  HCK(blk_scan(tmp, &tb, ucnt, uptr, nk + 1, c->st));
  int64_t units = 0;
  HCK(hipMemcpyAsync(&units, uptr + nk, sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
  sync(c);
  dfree(c, tmp);
  dfree_t(c, ucnt);
  if (units < ((int64_t)1 << 31)) {   // the kernel keeps record positions in 32 bits
    S.seg = dalloc<uint64_t>(c, units + 1);
    HCK(seg_scatter(c->rowptr, c->colidx, c->val, c->sp_f32, nrows, shift, cnt, first, uptr, S.seg, c->st));
    S.tptr = dalloc<int64_t>(c, m + 1);
    HCK(hipMemcpyAsync(S.tptr, tp.data(), sizeof(int64_t) * (m + 1), hipMemcpyHostToDevice, c->st));
    S.T = dalloc<uint64_t>(c, nT);
    HCK(seg_table(c->colptr, c->rowidx, cnt, uptr, nrows, m, shift, S.tptr, S.T, c->st));
    S.sw = dalloc<double>(c, nnz);
    S.shift = shift;
    S.state = 1;
  }
  sync(c);   // the temporaries' last readers
  dfree_t(c, cnt);
  dfree_t(c, first);
  dfree_t(c, uptr);
  return S.state > 0;
}

bool sparse_gram(scs_ctx* c) {
  if (!c->sparse) return false;
  if (const char* e = std::getenv("SCS_SPARSE_GRAM")) return e[0] == '1';   // read per call (A/B tests)
  if (c->sp_gram == 0) {
    std::vector<int64_t> rp((size_t)c->N + 1);
    HCK(hipMemcpyAsync(rp.data(), c->rowptr, sizeof(int64_t) * (c->N + 1), hipMemcpyDeviceToHost, c->st));
    sync(c);
    double s2 = 0.0;
    for (int64_t r = 0; r < c->N; ++r) s2 += (double)(rp[r + 1] - rp[r]) * (double)(rp[r + 1] - rp[r]);
    c->sp_gram = (64.0 * s2 <= (double)c->N * (double)c->dc * (double)c->dc) ? 1 : 2;
  }
  return c->sp_gram == 1;
}

// the sparse Gram -> out (upper part, ldg = m_pad), or packed 128 x 128 slots (multi-rank) through G
void gram_sparse(scs_ctx* c, const double* w, double* out, int packed) {
  double* dst = (packed & 1) ? c->G : out;
  if (packed & 2) fail(c, SCS_ERR_ARG, "internal: the sparse Gram does not accumulate");
  if (sparse_gram_requested() == 8 && build_gram_seg(c)) {   // variant 8 (default)
    const scs_ctx::SegGram& S = c->sgseg;
    HCK(csc_weight(c->rowidx, c->valT, c->sp_f32, w, c->nnz, S.sw, c->st));
    HCK(launch_sparse_gram_seg(c->colptr, S.sw, S.tptr, S.T, S.seg, c->sp_f32, c->dc, S.shift, dst, c->dcp, c->st));
    c->gram_kname = c->sp_f32 ? "sparse_gram_seg_kernel<float, 0>" : "sparse_gram_seg_kernel<double, 0>";   // rocprofv3's names
    if (packed & 1) HCK(gram_pack_launch(c->G, c->dcp, c->utiles, c->nslots, out, c->st));
    return;
  }
  if (!c->bgram.ptr) build_gram_blocked(c);
  HCK(launch_sparse_gram(c->colptr, c->rowidx, c->valT, c->bgram.ptr, c->bgram.lidx, c->bgram.val, c->bgram.nnz,
                         c->sp_f32, w, c->N, c->dc, c->bgram.shift, dst, c->dcp, c->st));
  c->gram_kname = sparse_gram_kernel_name(c->sp_f32, c->bgram.nnz);
  if (packed & 1) HCK(gram_pack_launch(c->G, c->dcp, c->utiles, c->nslots, out, c->st));
}

// How the Gram of a sparse A gets its dense operand tiles: a mirror of all of A when it fits
// under the cap (SCS_SPARSE_MIRROR_MAX_GB, default: the free device memory less the m x m
// system and 4 GiB), else the streaming ring (memory O(nnz + R·m + m²) for any N).
bool sparse_streams(scs_ctx* c) {
  if (!c->sparse) return false;
  if (c->sp_mode == 0) {
    const double bytes = (double)c->Npad * c->dcp * sizeof(double);   // the mirror of the data view
    size_t fr = 0, tot = 0;
    HCK(hipMemGetInfo(&fr, &tot));
    double cap = (double)fr - (double)c->mpad * c->mpad * 24 - 4.0 * 1073741824.0;
    if (const char* e = std::getenv("SCS_SPARSE_MIRROR_MAX_GB")) cap = std::atof(e) * 1073741824.0;
    c->sp_mode = (bytes <= cap) ? 1 : 2;
  }
  return c->sp_mode == 2;
}

// Streaming sparse Gram (Jt*Q*Jt' of a SparseMatrixCSC, prox-GGN-SCORE.jl:114,129 / a hess_fx Gram):
// rows are densified R at a time into one of two panel-blocked ring slots (the CSR scatter is
// O(nnz), the slot's previous chunk is cleared by scattering zeros at its own positions) and the
// production Gram launch accumulates each chunk's Aᵀ diag(w) A into G -- the MFMA tiles are the
// dense kernel's, K split into N/R chunks.
void gram_main_stream(scs_ctx* c, const double* w, double* out, int packed) {
  if (!c->ringA) {
    int64_t R = 0;
    if (const char* e = std::getenv("SCS_SPARSE_CHUNK_ROWS")) R = round_up(std::max<int64_t>(16, std::atoll(e)), 16);
    if (R == 0) {   // two slots within min(16 GiB, a quarter of the free memory)
      size_t fr = 0, tot = 0;
      HCK(hipMemGetInfo(&fr, &tot));
      const double budget = std::min(16.0 * 1073741824.0, 0.25 * (double)fr);
      R = std::max<int64_t>(2048, (int64_t)(budget / (2.0 * c->dcp * sizeof(double))) / 2048 * 2048);
    }
    c->ring_rows = std::min(R, c->Npad);
    c->ringA = dalloc<double>(c, (size_t)2 * c->ring_rows * c->dcp);
    c->ring_r0[0] = c->ring_r0[1] = -1;
  }
  const int64_t R = c->ring_rows;
  const int64_t nchunk = ceil_div(std::max<int64_t>(c->N, 1), R);
  for (int64_t k = 0; k < nchunk; ++k) {
    const int s = (int)(k & 1);
    double* slot = c->ringA + (size_t)s * R * c->dcp;
    const int64_t r0 = k * R, n = std::min(R, c->N - r0);
    if (c->ring_r0[s] >= 0)
      HCK(launch_densify_range(c->rowptr, c->colidx, c->val, c->sp_f32, c->ring_r0[s], c->ring_n[s], R, 1, slot, c->st));
    HCK(launch_densify_range(c->rowptr, c->colidx, c->val, c->sp_f32, r0, n, R, 0, slot, c->st));
    c->ring_r0[s] = r0;
    c->ring_n[s] = n;
    const int mode = packed | (k > 0 ? 2 : 0);
    const int64_t nk = round_up(std::max<int64_t>(n, 1), 16);   // w + r0 + nk <= w + Npad
    const bool pr = c->ptiles && !(packed & 1);   // unpacked: the paired list
    if (c->gwork)
      HCK(gram_launch_sched(slot, 0, R / 16, w + r0, nk, pr ? c->pwork : c->gwork, pr ? c->pseglen : c->gseglen,
                            pr ? c->pnsplit : c->gnsplit, pr ? c->pcomb : c->gcomb, pr ? c->pncomb : c->gncomb,
                            c->gpart, out, c->dcp, mode, c->tall, c->st));
    else
      HCK(gram_launch(slot, 0, R / 16, w + r0, nk, pr ? c->ptiles : c->tiles, pr ? c->nptiles : c->ntiles, out,
                      c->dcp, mode, c->tall, c->st));
    c->gram_kname = gram_main_kernel_name();
  }
}

// v != nullptr: the same launch forms Aᵀv of the local rows into vout (fused, gram_fuse_ok)
void gram_main(scs_ctx* c, const double* w, double* out, int packed, const double* v = nullptr,
               double* vout = nullptr) {
  if (sparse_gram(c)) {
    if (v) fail(c, SCS_ERR_ARG, "internal: the sparse Gram forms no Aᵀv");
    gram_sparse(c, w, out, packed);
    return;
  }
  if (sparse_streams(c)) {
    if (v) fail(c, SCS_ERR_ARG, "internal: the streaming sparse Gram forms no Aᵀv");
    gram_main_stream(c, w, out, packed);
    return;
  }
  const double* A = dense_A(c);
  const bool pr = c->ptiles && !(packed & 1);   // unpacked: the paired list
  const int nsplit = pr ? c->pnsplit : c->gnsplit;
  const int npiece = (v && c->gwork) ? std::max(nsplit, 1) : 1;
  if (v && npiece > 1) HCK(hipMemsetAsync(c->vpart, 0, sizeof(double) * npiece * c->dcp, c->st));
  if (c->gwork)
    HCK(gram_launch_sched(A, dense_a32(c), c->nstage, w, c->Npad, pr ? c->pwork : c->gwork,
                          pr ? c->pseglen : c->gseglen, nsplit, pr ? c->pcomb : c->gcomb, pr ? c->pncomb : c->gncomb,
                          c->gpart, out, c->dcp, packed, c->tall, c->st, v, c->vpart, c->dcp));
  else
    HCK(gram_launch(A, dense_a32(c), c->nstage, w, c->Npad, pr ? c->ptiles : c->tiles, pr ? c->nptiles : c->ntiles,
                    out, c->dcp, packed, c->tall, c->st, v, c->vpart, c->dcp));
  c->gram_kname = gram_main_kernel_name();
  if (v) HCK(gram_vfinal_launch(c->vpart, npiece, c->dcp, c->dc, vout, c->st));
}

// Gram of the local rows with weights w -> c->G (single rank) or the packed
// reduce buffer (multi-rank; then all-reduced together with `vec`).
// AᵀQA does not depend on x: least squares under ProxNSCORE (hess_fx = c·AᵀA) or under
// ProxGGNSCORE with the linear out_fn (J = A, Q = c·I); the reference still recomputes it every
// step (prox-GGN-SCORE.jl:129), which stays the default
bool gram_x_independent(const scs_ctx* c) {
  if (c->loss != SCS_LOSS_LEAST_SQUARES) return false;
  return c->method == SCS_PROX_NSCORE || (c->method == SCS_PROX_GGNSCORE && c->ggn == SCS_GGN_LINEAR_LS);
}

// vec_dev = Aᵀv of the local rows (then reduced with the Gram): formed inside the Gram launch
// (gram_sia_kernel AV) unless the Gram is served from the cache (a cached run never fuses, so
// its steps all take the same separate Aᵀv pass) or SCS_GRAM_FUSE=0
void gram_and_reduce(scs_ctx* c, const double* w, const double* v, double* vec_dev) {
  ensure_gram(c);
  ensure_red(c);
  hipEvent_t e0;
  const bool cacheable = c->gram_cache && gram_x_independent(c);
  const size_t gbytes = sizeof(double) * (size_t)c->mpad * c->mpad;
  // sparse A: Aᵀv from the CSC copy (a streaming Gram has no whole-A pass to ride on)
  const bool fuse = !cacheable && !c->sparse && gram_fuse_ok(c->tall);
  if (!fuse) gemv_t_local(c, v, vec_dev);
  if (cacheable && c->Gk && c->gk_gen == c->data_gen) {   // the reduced Gram of an earlier step
    c->g_from_cache = true;
    HCK(hipMemcpyAsync(c->G, c->Gk, gbytes, hipMemcpyDeviceToDevice, c->st));
    if (sharded(c)) {
      HCK(hipMemcpyAsync(c->red, vec_dev, sizeof(double) * c->m, hipMemcpyDeviceToDevice, c->st));
      allreduce(c, c->red, c->m);
      HCK(hipMemcpyAsync(vec_dev, c->red, sizeof(double) * c->m, hipMemcpyDeviceToDevice, c->st));
    }
    return;
  }
  if (sharded(c)) {
    const int64_t tsz = (int64_t)c->nslots * 128 * 128;
    tbegin(c, T_GRAM, &e0);
    gram_main(c, w, c->red, 1, fuse ? v : nullptr, vec_dev);
    tend(c, T_GRAM, e0);
    HCK(hipMemcpyAsync(c->red + tsz, vec_dev, sizeof(double) * c->m, hipMemcpyDeviceToDevice, c->st));
    allreduce(c, c->red, tsz + c->m);
    HCK(gram_unpack_launch(c->red, c->utiles, c->nslots, c->G, c->mpad, c->st));
    HCK(hipMemcpyAsync(vec_dev, c->red + tsz, sizeof(double) * c->m, hipMemcpyDeviceToDevice, c->st));
  } else {
    tbegin(c, T_GRAM, &e0);
    gram_main(c, w, c->G, 0, fuse ? v : nullptr, vec_dev);
    tend(c, T_GRAM, e0);
  }
  if (cacheable) {
    if (!c->Gk) c->Gk = dalloc<double>(c, (size_t)c->mpad * c->mpad);
    HCK(hipMemcpyAsync(c->Gk, c->G, gbytes, hipMemcpyDeviceToDevice, c->st));
    c->gk_gen = c->data_gen;
  }
}

// The factor hidden under the Gram (SCS_CHOL_PIPE=1; off by default, see below): one scheduled Gram launch per
// outer strip of the system on the context stream; on a second stream, as each strip lands:
// λ·Hr on its diagonal (and the padding's 1s), its copy into Gc (the LU fallback's system), the
// left-looking update from every earlier strip, its diagonal block and row strip
// (chol_strip_update / chol_strip_factor).  Only the last strip's factor and the two triangular
// solves remain after the Gram.  Single rank, dense A, Gram not served from the cache; m/128 >= 3
// outer blocks.  The result is the same factor up to the summation order of the updates
// (left- instead of right-looking).
// Measured at C2 (m = 8192, one box, same build): step 118.5 ms piped vs 107.7 ms classic.  The
// exposed solve drops 13.1 -> 6.2 ms, but the Gram grows 93.3 -> 110.9 ms: a strip launch is less
// than one round of the chip (strip 0: 484 tiles on 512 slots took 24.3 ms alone against its 21.5 ms
// share -- the interleaved kernel does not run a lone workgroup per CU twice as fast), and the
// factor's workgroups share CUs with MFMA-bound Gram waves (the left-looking updates ran at ~11 %
// of their alone rate).  At C3 (16 strips of 256 x 128 tiles) the partial rounds alone would cost
// seconds.  Hiding the factor needs the one-launch Gram with per-strip completion counters.
// SCS_CHOL_PIPE=2: ONE scheduled Gram launch whose per-XCD segments run the strips in order and
// count each finished tile into its strip; the factor stream waits for a strip's count
// (strip_wait_kernel) instead of an event after a per-strip launch, so the Gram keeps whole
// rounds.  (gram_factor_pipelined)
int pipe_mode(const scs_ctx* c, bool cacheable) {
  const char* e = std::getenv("SCS_CHOL_PIPE");   // read per step (tests toggle it in-process)
  const int mode = e ? std::atoi(e) : 0;
  const int64_t nblk = c->mpad / 128;
  const bool ok = !cacheable && !sharded(c) && !c->sparse && c->gwork && c->solver == 0 &&
                  nblk >= 3 * chol_outer_block();
  return ok && (mode == 1 || mode == 2) ? mode : 0;
}
bool pipe_ok(const scs_ctx* c, bool cacheable) { return pipe_mode(c, cacheable) != 0; }

// Gram (+ fused Aᵀv into vec_dev) and the factor of G + λ diag(Hr); Gc receives the system.
// Returns with the factor enqueued on c->st (info in c->cinfo).
hipEvent_t gram_factor_pipelined(scs_ctx* c, const double* w, const double* v, double* vec_dev) {
  const int64_t m = c->m, ld = c->mpad;
  const int nb = (int)(ld / 128), OB = chol_outer_block(), ns = (int)c->gstrip.size();
  HCK(chol_pipe_init(&c->caux, ld, c->st));
  if (!c->sf) {
    HCK(hipStreamCreateWithFlags(&c->sf, hipStreamNonBlocking));
    HCK(hipEventCreateWithFlags(&c->evfac, hipEventDisableTiming));
  }
  while ((int)c->evstrip.size() < ns + 1) {
    hipEvent_t e;
    HCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->evstrip.push_back(e);
  }
  const bool fuse = !c->sparse && gram_fuse_ok(c->tall);
  if (!fuse) gemv_t_local(c, v, vec_dev);
  const double* A = dense_A(c);
  if (fuse && c->vpieces > 1) HCK(hipMemsetAsync(c->vpart, 0, sizeof(double) * c->vpieces * ld, c->st));
  HCK(hipMemsetAsync(c->cinfo, 0, sizeof(int), c->st));
  const bool one = pipe_mode(c, false) == 2;
  if (one) HCK(hipMemsetAsync(c->gp_cnt, 0, sizeof(unsigned) * ns, c->st));
  hipEvent_t e0;
  tbegin(c, T_GRAM, &e0);
  // the factor stream starts after everything already on st (weights, smoother, info reset)
  HCK(hipEventRecord(c->evstrip[ns], c->st));
  HCK(hipStreamWaitEvent(c->sf, c->evstrip[ns], 0));
  if (one) {
    const scs_ctx::GStrip& g = c->gpipe;
    HCK(gram_launch_sched(A, dense_a32(c), c->nstage, w, c->Npad, g.work, g.seglen, g.nsplit, g.comb, g.ncomb, c->gpart,
                          c->G, ld, 0, c->tall, c->st, fuse ? v : nullptr, c->vpart, ld, c->gp_cnt, OB));
    HCK(hipEventRecord(c->evstrip[ns - 1], c->st));   // the last strip (and its combined pieces)
  } else {
    for (int s2 = 0; s2 < ns; ++s2) {
      const scs_ctx::GStrip& g = c->gstrip[s2];
      HCK(gram_launch_sched(A, dense_a32(c), c->nstage, w, c->Npad, g.work, g.seglen, g.nsplit, g.comb, g.ncomb, c->gpart,
                            c->G, ld, 0, c->tall, c->st, fuse ? v : nullptr, c->vpart, ld));
      HCK(hipEventRecord(c->evstrip[s2], c->st));
    }
  }
  tend(c, T_GRAM, e0);
  hipEvent_t es;
  tbegin(c, T_SOLVE, &es);   // the solve's share of the step: what runs after the Gram
  if (fuse) HCK(gram_vfinal_launch(c->vpart, c->vpieces, ld, m, vec_dev, c->st));
  for (int s2 = 0; s2 < ns; ++s2) {
    if (one && s2 + 1 < ns)
      HCK(strip_wait_launch(c->gp_cnt + s2, c->gp_target[s2], c->gp_flag, c->sf));
    else
      HCK(hipStreamWaitEvent(c->sf, c->evstrip[s2], 0));
    const int64_t r0 = (int64_t)s2 * OB * 128, r1 = std::min<int64_t>((int64_t)(s2 + 1) * OB * 128, ld);
    if (r0 < m) HCK(launch_diag_add(c->G + r0 * ld + r0, ld, std::min(r1, m) - r0, c->lam, c->Hr + r0, c->sf));
    HCK(chol_diag_pad(c->G, ld, std::max(r0, m), r1, c->sf));
    // strip rows [r0, r1), columns [r0, ld) -> Gc
    HCK(chol_copy_rows(c->Gc, c->G, ld, r0, r1, r0, ld, c->sf));
    HCK(chol_strip_update(c->G, ld, s2, &c->caux, c->sf));
    HCK(chol_strip_factor(c->G, ld, s2, c->W, &c->caux, c->trilist, c->cinfo, c->sf));
  }
  (void)nb;
  HCK(hipEventRecord(c->evfac, c->sf));
  HCK(hipStreamWaitEvent(c->st, c->evfac, 0));
  return es;
}

// fixed step-size rules shared by ProxNSCORE / ProxGGNSCORE
double step_size_newton(scs_ctx* c, int64_t iter, bool* needs_ls) {
  *needs_ls = false;
  if (c->ss_type == 1 && c->has_L) return jl_min_h(1 / c->L, 1.0);
  if (c->ss_type == 1 && !c->has_L) return 0.5;
  if (c->ss_type == 2) {
    if (iter == 1) return 1.0;
    // prox-N-SCORE.jl:81-83 / prox-GGN-SCORE.jl:78-80 call hμ.grad(x_prev) with one
    // argument and use an undefined ∇f: the reference raises a MethodError here.
    fail(c, SCS_ERR_REF, "MethodError: ss_type=2 calls hμ.grad(x_prev) with the wrong arity (reference bug, "
                         "prox-N-SCORE.jl:81 / prox-GGN-SCORE.jl:78)");
  }
  if (c->ss_type == 3) {
    *needs_ls = true;
    return 0.0;
  }
  fail(c, SCS_ERR_REF, "Please, choose ss_type in [1, 2, 3].");
}

// ggn_score_step's sample-space branch (prox-GGN-SCORE.jl:124-127, N + 1 <= m) -> c->d
void ggn_sample_direction(scs_ctx* c, const double* xh);

// The sample-space branch across ranks: its (N+1) x (N+1) system couples every pair of
// samples, so the ranks' rows are all-gathered once (each rank writes its rows into the
// zeroed reduce buffer at their global positions; the sum is the full A and y, at most
// N_global·m <= m² doubles -- the size of the feature branch's Gram exchange) and every
// rank runs the single-rank branch on that view, redundantly, as it does the m x m solve.
void ggn_sample_direction_sharded(scs_ctx* c, const double* xh) {
  if (c->sparse) fail(c, SCS_ERR_ARG, "the sharded GGN sample-space branch needs a dense A");
  ensure_red(c);
  const int64_t Ng = c->Nglob, Npg = round_up(std::max<int64_t>(Ng, 1), 16);
  const uint64_t gen = c->bsel < 0 ? 0 : c->batch_gen;
  const bool held = c->gview_ok && c->gview_batch == c->bsel && c->gview_gen == gen;
  if (c->gview_ok && !held && c->gview.N != Ng) {   // another size: new buffers
    free_view(c, c->gview);
    c->gview_ok = false;
  }
  if (!held) {
    ++c->y_stamp;   // the gathered view's y is refilled
    if (Npg * c->mpad + Npg > c->red_cap) fail(c, SCS_ERR_COMM, "reduce buffer too small for the row all-gather");
    // each local row at its global position: in the data (row0 + r) or in the selected batch
    std::vector<int64_t> rows(Ng, -1);
    if (c->bsel < 0) {
      for (int64_t r = 0; r < c->N; ++r) rows[c->row0 + r] = r;
    } else {
      const int64_t o = c->boff[c->bsel];
      for (int64_t r = 0; r < c->N; ++r) rows[c->bpos[o + r]] = r;
    }
    int64_t* drows = dalloc<int64_t>(c, Ng);
    HCK(hipMemcpyAsync(drows, rows.data(), sizeof(int64_t) * Ng, hipMemcpyHostToDevice, c->st));
    // (an fp32-stored A is widened into the fp64 reduce buffer: the gathered view is fp64, at most m x m)
    HCK(launch_gather_rows(c->A, c->a32, c->Npad, c->y, drows, Ng, Npg, c->mpad, c->red, 0, c->red + Npg * c->mpad,
                           c->st));
    allreduce(c, c->red, Npg * c->mpad + Npg);
    NView& v = c->gview;
    const bool fresh = !c->gview_ok;   // same size as the view held: refill its buffers in place
    if (fresh) {
      v.N = v.Nglob = Ng;
      v.Npad = Npg;
      v.nstage = Npg / 16;
      v.A = dalloc<double>(c, (size_t)Npg * c->mpad);
      v.y = dalloc<double>(c, Npg);
    }
    HCK(hipMemcpyAsync(v.A, c->red, sizeof(double) * Npg * c->mpad, hipMemcpyDeviceToDevice, c->st));
    HCK(hipMemcpyAsync(v.y, c->red + Npg * c->mpad, sizeof(double) * Npg, hipMemcpyDeviceToDevice, c->st));
    // a refilled view's Aᵀ copy (built once per A by ggn_sample_direction) follows its rows
    if (!fresh && v.At) HCK(launch_transpose(v.A, 0, v.Npad, Ng, c->m, v.At, c->mpad, v.ss.NpS, c->st));
    sync(c);
    dfree_t(c, drows);
    if (fresh) alloc_nspace(c, v);
    c->gview_ok = true;
    c->gview_batch = c->bsel;
    c->gview_gen = gen;
  }
  struct Scope {   // the gathered rows on one logical rank, restored even when the step fails
    scs_ctx* c;
    int nr;
    bool force;
    explicit Scope(scs_ctx* cc) : c(cc), nr(cc->nranks), force(cc->comm_force) {
      swap_view(c, c->gview);
      c->nranks = 1;
      c->comm_force = false;
      invalidate_caches(c);
    }
    ~Scope() {
      swap_view(c, c->gview);
      c->nranks = nr;
      c->comm_force = force;
      invalidate_caches(c);
    }
  } scope(c);
  ggn_sample_direction(c, xh);
}

// The sparse sample-space branch (scs_set_sparse_sample): P from the nonzeros, no mirror, no Aᵀ copy
bool sparse_sample_path(const scs_ctx* c) { return c->sparse_sample && c->sparse && !sharded(c); }

SampleSys& sample_sys(scs_ctx* c, int64_t N) {
  for (SampleSys& S : c->ssys)
    if (S.N == N) return S;
  c->ssys.emplace_back();   // filled in place: free_sample_sys gives a failed allocation's part back
  SampleSys& S = c->ssys.back();
  S.N = N;
  S.NpS = round_up(N, 128);
  S.n1pad = round_up(N + 1, 128);
  S.Ps = dalloc<double>(c, (size_t)S.NpS * S.NpS);
  S.Ms = dalloc<double>(c, (size_t)S.n1pad * S.n1pad);
  S.bS = dalloc<double>(c, S.n1pad);
  S.uN = dalloc<double>(c, round_up(std::max<int64_t>(N, 1), 16));
  S.hvec = dalloc<double>(c, c->mpad);
  S.hg = dalloc<double>(c, c->mpad);
  return S;
}

// The Gram-blocked copy of the CSC (the column side of build_gram_blocked): the sorted columns cut
// into 2^sparse_gram_shift()-wide blocks of rows, unpadded.  A batch view brings its own.
void build_sample_blocked(scs_ctx* c) {
  SpBlkT& B = c->sgram;
  const int64_t ncols = c->m;
  B.shift = sparse_gram_shift();
  B.nblk = (int)std::max<int64_t>(ceil_div(c->N, int64_t(1) << B.shift), 1);
  const int64_t nk = (int64_t)B.nblk * ncols;
  int64_t* cnt = dalloc<int64_t>(c, nk + 1);
  int64_t* first = dalloc<int64_t>(c, nk + 1);
  B.ptr = dalloc<int64_t>(c, nk + 1);
  HCK(blk_count(c->colptr, c->rowidx, ncols, B.shift, cnt, first, c->st));
  size_t tb = 0;
  HCK(blk_scan(nullptr, &tb, cnt, B.ptr, nk + 1, c->st));
  void* tmp = dalloc<char>(c, tb);
  HCK(blk_scan(tmp, &tb, cnt, B.ptr, nk + 1, c->st));
  int64_t nnz = 0;
  HCK(hipMemcpyAsync(&nnz, B.ptr + nk, sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
  sync(c);
  dfree(c, tmp);
  B.nnz = nnz;
  B.lidx = dalloc<uint16_t>(c, nnz + 8);
  B.val = c->sp_f32 ? (void*)dalloc<float>(c, (size_t)nnz + 8) : (void*)dalloc<double>(c, (size_t)nnz + 8);
  HCK(blk_scatter(c->colptr, c->rowidx, c->valT, c->sp_f32, ncols, B.shift, B.ptr, first, B.lidx, B.val, c->st));
  sync(c);
  dfree_t(c, cnt);
  dfree_t(c, first);
}

// P = A diag(h) Aᵀ (upper triangle, ld NpS) of the sparse rows in place, from their nonzeros
void sparse_sample_gram(scs_ctx* c, const double* h, double* Ps, int64_t NpS) {
  // (the shift is read per call for A/B tests; a batch view in place keeps the shift it was built with)
  if (c->spview >= 0 && !c->sgram.ptr) fail(c, SCS_ERR_STATE, "internal: this batch view holds no sample-space copy");
  if (!c->sgram.ptr || (c->spview < 0 && c->sgram.shift != sparse_gram_shift())) {
    sync(c);
    free_blk(c, c->sgram);
    build_sample_blocked(c);
  }
  const SpBlkT& B = c->sgram;
  HCK(launch_sparse_sample_gram(c->rowptr, c->colidx, c->val, B.ptr, B.lidx, B.val, B.nnz, c->sp_f32, h, c->N, c->m,
                                B.shift, Ps, NpS, c->st));
  c->gram_kname = sparse_sample_kernel_name(c->sp_f32, B.nnz);
}

// The sample-space system M B = b solved in place (Ms row-major, order n1, padded order np1; bS <- B):
// a non-finite system gives a NaN solution, the reference-solver mode runs the QR, else the LU with
// `rebuild` (the system assembled again) as its redo.  Under T_SOLVE.
template <class F>
void sample_space_solve(scs_ctx* c, double* Ms, int64_t np1, int64_t n1, double* bS, F&& rebuild) {
  hipEvent_t e0;
  tbegin(c, T_SOLVE, &e0);
  int info = 0;
  // NaN / Inf in the system: the reference's qr(...) \ b comes out NaN (no SingularException)
  HCK(hipMemsetAsync(c->cinfo, 0, sizeof(int), c->st));
  HCK(launch_nonfinite(Ms, np1, n1, bS, c->cinfo, c->st));
  HCK(hipMemcpyAsync(&info, c->cinfo, sizeof(int), hipMemcpyDeviceToHost, c->st));
  sync(c);
  if (info != 0) {
    HCK(launch_fill(bS, n1, std::numeric_limits<double>::quiet_NaN(), c->st));
  } else if (c->solver == SCS_SOLVER_REFERENCE) {
    // qr(I + A) \ residual (prox-GGN-SCORE.jl:126): the row-major system transposed into a
    // column-major copy with identity padding, Householder QR
    if (c->qrM_n != np1) {
      dfree_t(c, c->qrM);
      c->qrM = dalloc<double>(c, (size_t)np1 * np1);
      c->qrM_n = np1;
    }
    HCK(qr_from_rowmajor(Ms, np1, c->qrM, np1, n1, np1, c->st));
    qr_run(c, &c->qr, c->qbk, c->qbk_n, c->qrM, np1, bS);
  } else {
    HCK(lu_aux_init(&c->lu, np1, c->st));
    info = lu_factor_checked(c, Ms, np1, n1, np1, c->cinfo, rebuild);
    if (info != 0) fail(c, SCS_ERR_SOLVE, "SingularException(%d)", info);
    HCK(lu_solve(Ms, np1, np1, &c->lu, bS, c->st));
  }
  tend(c, T_SOLVE, e0);
}

// The system of the branch at x (c->x, smoother evaluated): the forward pass, P = A diag(h) Aᵀ, u and the
// assembly into S.Ms / S.bS (row-major, order N + 1, padded order S.n1pad) -- everything before the solve
const SampleSys& ggn_sample_system(scs_ctx* c, const double* xh) {
  const int64_t N = c->N, m = c->m;
  const bool sps = sparse_sample_path(c);
  if (!sps && c->At && c->loss == SCS_LOSS_CALLBACK)   // the caller's J changes every step
    HCK(launch_transpose(c->A, c->a32, c->Npad, N, m, c->At, c->mpad, c->ss.NpS, c->st));
  if (!sps && !c->At) {
    const double* A = dense_A(c);
    SampleSys& O = c->ss;   // the view's own system scratch
    O.NpS = round_up(N, 128);
    c->At = dalloc<double>(c, (size_t)O.NpS * c->mpad);
    HCK(launch_transpose(A, dense_a32(c), c->Npad, N, m, c->At, c->mpad, O.NpS, c->st));
    O.Ps = dalloc<double>(c, (size_t)O.NpS * O.NpS);
    O.n1pad = round_up(N + 1, 128);   // row-major, zero padding (lu.hip)
    O.Ms = dalloc<double>(c, (size_t)O.n1pad * O.n1pad);
    O.bS = dalloc<double>(c, O.n1pad);
    O.uN = dalloc<double>(c, c->Npad);
    O.hvec = dalloc<double>(c, c->mpad);
    O.hg = dalloc<double>(c, c->mpad);
    const int nb = (int)(O.NpS / 128);
    std::vector<int2> tl((size_t)nb * (nb + 1) / 2);
    int nt = 0;
    gram_tile_list(nb, tl.data(), &nt);
    c->stiles = dalloc<int2>(c, nt);
    HCK(hipMemcpyAsync(c->stiles, tl.data(), sizeof(int2) * nt, hipMemcpyHostToDevice, c->st));
    c->nstiles = nt;
  }
  // the system scratch: the view's own, or (sparse branch) the set kept for this size
  const SampleSys& S = sps ? sample_sys(c, N) : c->ss;
  double *const Ps = S.Ps, *const Ms = S.Ms, *const bS = S.bS, *const uN = S.uN, *const hvec = S.hvec, *const hg = S.hg;
  const int64_t NpS = S.NpS, n1pad = S.n1pad;
  // s, q, r (prox-GGN-SCORE.jl:44-56) -> gN, hN, wN (a callback loss filled them: ggn_cb_load)
  if (c->loss != SCS_LOSS_CALLBACK) forward(c, xh, c->x, EPI_GGN | EPI_SQR, false);
  HCK(launch_ggn_sample_prep(c->Hr, c->gr, c->lam, m, c->mpad, hvec, hg, c->st));
  hipEvent_t e0;
  tbegin(c, T_GRAM, &e0);
  if (sps)
    sparse_sample_gram(c, hvec, Ps, NpS);
  else
    HCK(gram_launch_gen(c->At, c->mpad, c->At, c->mpad, hvec, 0, c->mpad, c->stiles, c->nstiles, Ps, NpS,
                        /*GRAM_UPPER*/ 4, c->st));
  tend(c, T_GRAM, e0);
  HCK(launch_symmetrize(Ps, NpS, N, c->st));
  const int ns = matvec_n(c, hg, c->nsplit);   // u = A (h∘λgr)
  HCK(launch_epilogue(SCS_LOSS_LEAST_SQUARES, SCS_GGN_NONE, EPI_Z, c->zpart, ns, c->Npad, c->y, N, c->Npad, 1.0,
                      uN, nullptr, nullptr, nullptr, nullptr, c->valpart, c->st));
  HCK(launch_ggn_sample_assemble(Ps, NpS, c->gN, c->hN, c->wN, uN, nullptr, N, Ms, n1pad, bS,
                                      c->st));
  return S;
}

void ggn_sample_direction(scs_ctx* c, const double* xh) {
  const int64_t N = c->N, m = c->m;
  if (sharded(c)) return ggn_sample_direction_sharded(c, xh);
  const SampleSys& S = ggn_sample_system(c, xh);
  sample_space_solve(c, S.Ms, S.n1pad, N + 1, S.bS, [&] {   // the system assembled again
    HCK(launch_ggn_sample_assemble(S.Ps, S.NpS, c->gN, c->hN, c->wN, S.uN, nullptr, N, S.Ms, S.n1pad, S.bS,
                                   c->st));
  });
  HCK(launch_ggn_sample_scale(c->gN, S.bS, N, c->Npad, c->vN, c->st));
  gemv_t_local(c, c->vN, c->gtmp);   // Aᵀ(s∘B)
  HCK(launch_ggn_sample_direction(S.hvec, c->gtmp, S.hg, S.bS, N, m, c->d, c->st));
}

// host column-major rows (N x m, lda) -> panel-blocked dst (Npad x mpad), one 128-column panel
// at a time through the column-major staging buffer C (Npad x 128).  in32: the host rows (and C's
// elements) are float; a32: dst's are -- fp64 rows into an fp32 dst are rounded in the retile step
static void upload_panels(scs_ctx* c, const void* A, int in32, int64_t N, int64_t lda, int64_t Npad, double* dst,
                          int a32, double* C) {
  const int64_t m = c->dc;
  const size_t es = in32 ? sizeof(float) : sizeof(double);
  for (int64_t p = 0; p < c->dcp / 128; ++p) {
    const int64_t j0 = p * 128, nc = std::min<int64_t>(128, m - j0);
    HCK(hipMemsetAsync(C, 0, es * Npad * 128, c->st));
    if (nc > 0 && N > 0)
      HCK(hipMemcpy2DAsync(C, es * Npad, (const char*)A + es * j0 * lda, es * lda, es * N, nc, hipMemcpyHostToDevice,
                           c->st));
    HCK(launch_retile(C, in32, dst, a32, Npad, p, 1, c->st));
  }
}

// ProxGGNSCORE on a callback loss (jac_yx / grad_fy / hess_fy, prox-GGN-SCORE.jl:44-49): the
// caller hands over J (n x m, column-major), r and the diagonal q of Q (a general symmetric Q
// arrives eigen-rotated: J̃ = VᵀJ, r̃ = Vᵀr, q = eigenvalues -- JᵀQJ, Jᵀr and the sample-space
// system are unchanged).  J is uploaded into the callback view, which then stands in for the
// data with s = 1: w = q, v = r in the feature branch; (s, q, r) = (1, q, r) in the sample one.
void ggn_cb_load(scs_ctx* c, const double* xh, bool sample) {
  const int64_t n = c->cb_nout, m = c->m;
  const double* out = cb_eval(c, SCS_CB_GGN, xh, c->x, (size_t)n * (m + 2));
  NView& v = c->cbv;
  if (!v.A) {
    v.N = v.Nglob = n;
    v.Npad = round_up(std::max<int64_t>(n, 1), 16);
    v.nstage = v.Npad / 16;
    v.A = dalloc<double>(c, (size_t)v.Npad * c->mpad);
    v.y = dalloc<double>(c, v.Npad);
    alloc_nspace(c, v);
    c->cbstage = dalloc<double>(c, (size_t)v.Npad * 128);
  }
  upload_panels(c, out, 0, n, n, v.Npad, v.A, 0, c->cbstage);
  const double* r = out + (size_t)n * m;
  const double* q = r + n;
  if (sample) {
    HCK(launch_fill(v.gN, n, 1.0, c->st));
    HCK(hipMemcpyAsync(v.hN, q, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
    HCK(hipMemcpyAsync(v.wN, r, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
  } else {
    HCK(hipMemcpyAsync(v.wN, q, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
    HCK(hipMemcpyAsync(v.vN, r, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
  }
}

// the callback view in place of the (absent) data for one GGN step, restored even on failure
struct CbScope {
  scs_ctx* c;
  explicit CbScope(scs_ctx* cc) : c(cc) {
    swap_view(c, c->cbv);
    c->generic = false;
    invalidate_caches(c);
  }
  ~CbScope() {
    swap_view(c, c->cbv);
    c->generic = true;
    invalidate_caches(c);
  }
};

// The Hessians written straight into G (Rosenbrock, a callback's hess_fx, the quadratic loss) fill
// its leading m x m block only and rely on the padded rows / columns being block-diag(H, I).  A
// Cholesky that met a non-positive pivot (an indefinite system: the LU then solves the copy) runs on
// through NaN pivots and leaves NaN in the padded columns of the rows it touched, which the next
// step's factor and LU would carry into every entry of the direction: clear the padding first (a
// Gram launch rewrites all of G, so the data losses never saw this).
static void clear_gram_padding(scs_ctx* c) {
  const int64_t m = c->m, ld = c->mpad;
  if (ld == m) return;
  HCK(hipMemsetAsync(c->G + m * ld, 0, sizeof(double) * (size_t)(ld - m) * ld, c->st));   // columns >= m
  HCK(hipMemset2DAsync(c->G + m, sizeof(double) * ld, 0, sizeof(double) * (ld - m), m, c->st));   // rows >= m
}

// ProxGGNSCORE on a multi-output context takes the feature branch only: with N·K + 1 <= d·K the
// reference's sample-space branch (prox-GGN-SCORE.jl:124-127) gives another step
bool multi_sample_shape(const scs_ctx* c) { return multi(c) && c->Nglob * c->nout + 1 <= c->m; }

// ... unless scs_set_multi_sample is on: multi_sample_direction then runs that branch on a dense A
void refuse_multi_sample_space(scs_ctx* c, int method) {
  if (!multi_sample_shape(c) || method != SCS_PROX_GGNSCORE) return;
  if (c->multi_sample) {
    if (c->sparse)
      fail(c, SCS_ERR_ARG, "ProxGGNSCORE with scs_set_outputs (nout = %d) at N*nout + 1 = %lld <= d*nout = %lld: the "
                           "sample-space branch of multi_sample / scs_set_multi_sample needs a dense A (a sparse A, "
                           "scs_set_sparse_outputs included, is not supported there) -- use the callback loss "
                           "(losses.callback) for this shape", c->nout, (long long)(c->Nglob * c->nout + 1),
           (long long)c->m);
    return;
  }
  fail(c, SCS_ERR_ARG, "ProxGGNSCORE with scs_set_outputs (nout = %d): N*nout + 1 = %lld <= d*nout = %lld, where the "
                       "reference takes its sample-space branch (H^-1 = 1/Hr without lambda: another step); the "
                       "multi-output device path forms the feature branch only -- use the callback loss "
                       "(losses.callback) for this shape", c->nout, (long long)(c->Nglob * c->nout + 1),
       (long long)c->m);
}

// The order-d·K system of a multi-output loss at the point of the last forward(EPI_GGN) (P in hN, s in
// vN): block (k, l) of JᵀQJ = ∇²f is Aᵀ diag(w_kl) A.  One weight vector at a time (never all
// K(K+1)/2), the unchanged weighted Gram into Gd, then its placement as blocks (k, l) and (l, k).
// Multi-target least squares: one Gram c·AᵀA on the K diagonal blocks, exact zeros elsewhere.
void multi_system(scs_ctx* c) {
  ensure_gram(c);
  const int K = c->nout;
  const int64_t ld = c->mpad;
  hipEvent_t e0;
  tbegin(c, T_GRAM, &e0);
  if (c->loss == SCS_LOSS_MULTI_LS) {
    HCK(hipMemsetAsync(c->G, 0, sizeof(double) * (size_t)ld * ld, c->st));
    HCK(launch_multi_weight(c->loss, c->hN, c->vN, 0, 0, c->N, c->Npad, c->scale, c->wN, c->st));
    gram_main(c, c->wN, c->Gd, 0);
    for (int k = 0; k < K; ++k) HCK(launch_multi_place(c->Gd, c->dcp, c->dc, k, k, c->G, ld, c->st));
  } else {
    clear_gram_padding(c);
    for (int k = 0; k < K; ++k)
      for (int l = k; l < K; ++l) {
        HCK(launch_multi_weight(c->loss, c->hN, c->vN, k, l, c->N, c->Npad, c->scale, c->wN, c->st));
        gram_main(c, c->wN, c->Gd, 0);
        HCK(launch_multi_place(c->Gd, c->dcp, c->dc, k, l, c->G, ld, c->st));
      }
  }
  tend(c, T_GRAM, e0);
}

// ---- ProxGGNSCORE's sample-space branch of a multi-output loss (scs_set_multi_sample) ----
// The view's sample-space fields hold its data: At the d-column transpose (NpS x dcp), ss.Ps one N x N
// P_l at a time, ss.Ms the row-major system of order N·K + 1, ss.uN the K vectors u_l (then V),
// ss.hvec the K padded weight slices h_l (dcp each), ss.hg = h ∘ λ gr in vec layout.
void multi_sample_setup(scs_ctx* c) {
  if (c->At) return;
  if (c->sparse) fail(c, SCS_ERR_ARG, "the multi-output sample-space branch (multi_sample) needs a dense A");
  free_buffers(c, *c, VB_SAMPLE);   // (what an allocation that failed half way left)
  c->nstiles = 0;
  const int64_t N = c->N, K = c->nout;
  SampleSys& O = c->ss;
  O.N = N;
  O.NpS = round_up(N, 128);
  O.n1pad = round_up(N * K + 1, 128);   // row-major, zero padding (lu.hip)
  O.Ps = dalloc<double>(c, (size_t)O.NpS * O.NpS);
  O.Ms = dalloc<double>(c, (size_t)O.n1pad * O.n1pad);
  O.bS = dalloc<double>(c, O.n1pad);
  O.uN = dalloc<double>(c, (size_t)c->Npad * K);
  O.hvec = dalloc<double>(c, (size_t)c->dcp * K);
  O.hg = dalloc<double>(c, c->mpad);
  const int nb = (int)(O.NpS / 128);
  std::vector<int2> tl((size_t)nb * (nb + 1) / 2);
  int nt = 0;
  gram_tile_list(nb, tl.data(), &nt);
  c->stiles = dalloc<int2>(c, nt);
  HCK(hipMemcpyAsync(c->stiles, tl.data(), sizeof(int2) * nt, hipMemcpyHostToDevice, c->st));
  c->nstiles = nt;
  double* At = dalloc<double>(c, (size_t)O.NpS * c->dcp);
  HCK(launch_transpose(c->A, c->a32, c->Npad, N, c->dc, At, c->dcp, O.NpS, c->st));
  sync(c);   // (the tile list's host copy goes out of scope)
  c->At = At;
}

// The column blocks of the system at the point of the last forward(EPI_GGN): per l the Gram P_l (the
// single-output launch on At with the weights h_l), its mirror, one assembly launch; then the tail.
// time_asm (the door): the assembly and tail launches are bracketed under T_STEP, which no step is using
void multi_sample_assemble(scs_ctx* c, bool time_asm = false) {
  const SampleSys& S = c->ss;
  const int K = c->nout;
  hipEvent_t e0;
  for (int l = 0; l < K; ++l) {
    tbegin(c, T_GRAM, &e0);
    HCK(gram_launch_gen(c->At, c->dcp, c->At, c->dcp, S.hvec + (int64_t)l * c->dcp, 0, c->dcp, c->stiles, c->nstiles,
                        S.Ps, S.NpS, /*GRAM_UPPER*/ 4, c->st));
    tend(c, T_GRAM, e0);
    HCK(launch_symmetrize(S.Ps, S.NpS, c->N, c->st));
    if (time_asm) tbegin(c, T_STEP, &e0);
    HCK(launch_multi_sample_assemble(c->loss, K, l, S.Ps, S.NpS, c->hN, c->vN, c->N, c->Npad, c->scale, S.Ms, S.n1pad,
                                     c->st));
    if (time_asm) tend(c, T_STEP, e0);
  }
  if (time_asm) tbegin(c, T_STEP, &e0);
  HCK(launch_multi_sample_tail(c->loss, K, c->hN, c->vN, S.uN, c->gN, c->N, c->Npad, c->scale, S.Ms, S.n1pad, S.bS,
                               c->st));
  if (time_asm) tend(c, T_STEP, e0);
}

// forward pass (P -> hN, s -> vN, R -> gN), h and h ∘ λ gr, the K vectors u_l in one pass over A, the system
void multi_sample_system(scs_ctx* c, const double* xh, bool time_asm = false) {
  multi_sample_setup(c);
  const SampleSys& S = c->ss;
  const int K = c->nout;
  forward(c, xh, c->x, EPI_GGN, false);
  HCK(launch_multi_sample_prep(c->Hr, c->gr, c->lam, c->dc, c->dcp, K, S.hvec, S.hg, c->st));
  hipEvent_t e0;
  tbegin(c, T_GEMV, &e0);
  const int ns = matvec_n(c, S.hg, c->nsplit);   // U = A reshape(h ∘ λ gr, d, K)
  tend(c, T_GEMV, e0);
  HCK(launch_multi_epilogue(SCS_LOSS_MULTI_LS, EPI_Z, K, c->zpart, ns, nullptr, c->N, c->Npad, 1.0, S.uN, nullptr,
                            nullptr, nullptr, nullptr, c->st));
  multi_sample_assemble(c, time_asm);
}

void multi_sample_direction(scs_ctx* c, const double* xh) {
  multi_sample_system(c, xh);
  const SampleSys& S = c->ss;
  const int K = c->nout;
  const int64_t n = c->N * K;
  sample_space_solve(c, S.Ms, S.n1pad, n + 1, S.bS, [&] { multi_sample_assemble(c); });
  HCK(launch_multi_sample_spread(S.bS, c->N, c->Npad, K, S.uN, c->st));
  gemv_t_local(c, S.uN, c->gtmp);   // vec(Aᵀ V), V = reshape(B[0 : N·K], N, K): one pass over A
  HCK(launch_multi_sample_direction(S.hvec, c->gtmp, S.hg, S.bS, n, c->dc, c->dcp, K, c->d, c->st));
}

// ProxNSCORE / ProxGGNSCORE direction of a multi-output loss -> c->d.  ∇²f = JᵀQJ (J = I_K ⊗ A, the
// output is linear in x), so both methods build the same system; rhs = vec(AᵀR) + λ gr.
void multi_newton_direction(scs_ctx* c, const double* xh) {
  const int64_t m = c->m;
  refuse_multi_sample_space(c, c->method);
  if (c->method == SCS_PROX_GGNSCORE && c->ggn == SCS_GGN_NONE)
    fail(c, SCS_ERR_ARG, "ProxGGNSCORE needs an out_fn / GGN loss kind");
  if (c->method == SCS_PROX_GGNSCORE && multi_sample_shape(c)) return multi_sample_direction(c, xh);
  forward(c, xh, c->x, EPI_GGN, false);
  gemv_t_local(c, c->gN, c->gtmp);
  if (c->gfix && c->method == SCS_PROX_NSCORE) grad_f_dev(c, xh, c->x, c->gtmp);
  multi_system(c);
  HCK(launch_axpby(c->gtmp, c->lam, c->gr, m, c->gq, c->st));
  HCK(launch_diag_add(c->G, c->mpad, m, c->lam, c->Hr, c->st));
  solve_system(c, c->gq);
  HCK(launch_neg(c->gq, m, c->d, c->st));
}

// ProxNSCORE / ProxGGNSCORE step
void step_newton(scs_ctx* c, const double* xh, int64_t iter, double* x_new, double* dx, double* pri) {
  const int64_t m = c->m;
  c->g_from_cache = false;
  HCK(launch_smoother(c->smooth, c->x, m, c->mu, c->slb, c->sub, c->wel, c->gr, c->Hr, c->st));
  const bool cbggn = c->method == SCS_PROX_GGNSCORE && c->loss == SCS_LOSS_CALLBACK;
  const bool sample_space = (c->method == SCS_PROX_GGNSCORE) &&
                            (cbggn ? c->cb_nout + 1 <= m : (c->Nglob + 1 <= m && c->ggn != SCS_GGN_NONE));
  if (cbggn) ggn_cb_load(c, xh, sample_space);
  // a sparse batch view holds what the sample space reads, not the m x m Gram's arrays
  if (c->spview >= 0 && !sample_space) fail(c, SCS_ERR_STATE, "a sparse batch view serves the GGN sample-space branch only");
  if (multi(c)) {
    multi_newton_direction(c, xh);
  } else if (sample_space) {
    if (cbggn) {
      CbScope scope(c);
      ggn_sample_direction(c, xh);
    } else {
      ggn_sample_direction(c, xh);
    }
  } else {
  ensure_gram(c);
  if (c->method == SCS_PROX_NSCORE) {
    // H = hess_fx, ∇q = grad_fx + λ gr  (prox-N-SCORE.jl:183-204)
    if (c->loss == SCS_LOSS_ROSENBROCK) {
      clear_gram_padding(c);
      HCK(launch_rosen(c->x, m, 2, nullptr, c->G, c->mpad, c->st));
      HCK(launch_rosen(c->x, m, 1, c->gtmp, nullptr, 0, c->st));
    } else if (c->loss == SCS_LOSS_CALLBACK) {
      // H = hess_fx(x) (m x m, column-major) into the leading block of G; the padded rows /
      // columns keep block-diag(H, I) (zero from the allocation and clear_gram_padding, the padded
      // diagonal set by chol_factor)
      const double* H = cb_eval(c, SCS_CB_HESS, xh, c->x, (size_t)m * m);
      clear_gram_padding(c);
      HCK(hipMemcpy2DAsync(c->G, sizeof(double) * c->mpad, H, sizeof(double) * m, sizeof(double) * m, m,
                           hipMemcpyHostToDevice, c->st));
      grad_f_dev(c, xh, c->x, c->gtmp);
    } else if (c->loss == SCS_LOSS_QUADRATIC) {
      require_dense(c, "the quadratic loss");
      clear_gram_padding(c);
      HCK(launch_half_sym(c->A, c->nstage, m, c->G, c->mpad, c->st));   // fp64 A only (require_dense)
      grad_f_dev(c, xh, c->x, c->gtmp);
    } else {
      forward(c, xh, c->x, EPI_GRAD | EPI_HESS, false);
      // local Aᵀg (not yet reduced; fused into the Gram pass); reduced together with the Gram
      if (pipe_ok(c, c->gram_cache && gram_x_independent(c))) {
        ensure_gram(c);
        const hipEvent_t es = gram_factor_pipelined(c, c->hN, c->gN, c->gtmp);
        if (c->gfix) grad_f_dev(c, xh, c->x, c->gtmp);   // ∇fx replaces the fused Aᵀg
        HCK(launch_axpby(c->gtmp, c->lam, c->gr, m, c->gq, c->st));
        if (solve_factored(c, c->gq, es)) {
          HCK(launch_neg(c->gq, m, c->d, c->st));
          goto newton_tail;
        }
        // (a strip wait gave up: the unpipelined Gram, factor and solve below)
      }
      gram_and_reduce(c, c->hN, c->gN, c->gtmp);
    }
  } else if (cbggn) {
    CbScope scope(c);
    gram_and_reduce(c, c->wN, c->vN, c->gtmp);   // JᵀQJ + Jᵀr of the caller's J (w = q, v = r)
  } else {
    if (c->ggn == SCS_GGN_NONE) fail(c, SCS_ERR_ARG, "ProxGGNSCORE needs an out_fn / GGN loss kind");
    // J, residual, Q (prox-GGN-SCORE.jl:44-56) -> w = s²q, v = s·r
    forward(c, xh, c->x, EPI_GGN, false);
    if (pipe_ok(c, c->gram_cache && gram_x_independent(c))) {
      ensure_gram(c);
      const hipEvent_t es = gram_factor_pipelined(c, c->wN, c->vN, c->gtmp);
      HCK(launch_axpby(c->gtmp, c->lam, c->gr, m, c->gq, c->st));
      if (solve_factored(c, c->gq, es)) {
        HCK(launch_neg(c->gq, m, c->d, c->st));
        goto newton_tail;
      }
      // (a strip wait gave up: the unpipelined Gram, factor and solve below)
    }
    gram_and_reduce(c, c->wN, c->vN, c->gtmp);   // Gram + Jᵀr in one pass over A
  }
  // rhs = ∇f + λ gr (NSCORE) | Jᵀr + λ gr (GGN: Jt*[r;1], prox-GGN-SCORE.jl:121-130); a caller's
  // ∇fx replaces ∇f in ProxNSCORE (prox-N-SCORE.jl:66-69; ProxGGNSCORE takes no ∇fx)
  if (c->gfix && c->method == SCS_PROX_NSCORE) grad_f_dev(c, xh, c->x, c->gtmp);
  HCK(launch_axpby(c->gtmp, c->lam, c->gr, m, c->gq, c->st));
  HCK(launch_diag_add(c->G, c->mpad, m, c->lam, c->Hr, c->st));
  solve_system(c, c->gq);
  HCK(launch_neg(c->gq, m, c->d, c->st));  // d = -sol
  }
newton_tail:
  bool ls = false;
  double step = step_size_newton(c, iter, &ls);
  if (ls) step = line_search(c, xh, c->x, c->d);
  const double Mg = get_Mg(c, c->Mh, c->nu, c->mu, m);
  HCK(launch_score_tail(c->x, c->d, c->gr, c->Hr, m, c->lam, Mg, step, nullptr, prox_args(c), c->hinv, c->zb, c->xn,
                        c->dxv, c->scal, c->st));
  if (c->dev_loop) return;   // x_new stays in c->xn, pri_res_norm in scal[0]
  d2h(c, x_new, c->xn, m);
  if (dx) d2h(c, dx, c->dxv, m);
  d2h(c, c->hscal, c->scal, 4);
  sync(c);
  *pri = c->hscal[0];
}

// L-BFGS memory update decision (prox-L-BFGS-SCORE.jl:154-162) from the device's δhᵀγh, γhᵀγh:
// accept the pair written to `slot` when δhᵀγh > 1e-10 (absolute), FIFO capped at mem
void lbfgs_accept(scs_ctx* c, int slot, double dg, double gg) {
  if (!(dg > 1e-10)) return;
  if ((int)c->ring.size() == c->mem) {
    c->spare = c->ring.front();
    c->ring.erase(c->ring.begin());
  } else {
    // the next unused physical slot becomes the spare
    std::vector<bool> used(c->mem + 1, false);
    for (int r : c->ring) used[r] = true;
    used[slot] = true;
    for (int i = 0; i <= c->mem; ++i)
      if (!used[i]) {
        c->spare = i;
        break;
      }
  }
  c->ring.push_back(slot);
  c->H0 = dg / gg;
}

// a memory update left in flight by the device loop: its dg / gg are in hscal[16..17] once the
// epoch-end copy has landed (scs_iterate syncs before calling this)
void lbfgs_settle(scs_ctx* c, bool synced) {
  if (!c->lbfgs_pending) return;
  if (!synced) {
    d2h(c, c->hscal + 16, c->scal + 16, 2);
    sync(c);
  }
  c->lbfgs_pending = false;
  lbfgs_accept(c, c->lbfgs_slot, c->hscal[16], c->hscal[17]);
}

// ProxLQNSCORE step (prox-L-BFGS-SCORE.jl:69-169)
void step_lqn(scs_ctx* c, const double* xh, const double* xph, int64_t iter, double* x_new, double* dx,
              double* pri) {
  const int64_t m = c->m;
  lbfgs_settle(c, false);
  HCK(launch_smoother(c->smooth, c->x, m, c->mu, c->slb, c->sub, c->wel, c->gr, c->Hr, c->st));
  grad_q_dev(c, xh, c->x, c->gq);  // ∇q = grad_f(x) + λgr
  const int k = (int)c->ring.size();
  if (iter == 1 || k == 0) {
    HCK(launch_neg(c->gq, m, c->d, c->st));
  } else {
    std::memcpy(c->hring, c->ring.data(), sizeof(int) * k);   // pinned: a truly asynchronous upload
    HCK(hipMemcpyAsync(c->d_order, c->hring, sizeof(int) * k, hipMemcpyHostToDevice, c->st));
    HCK(launch_two_loop(c->S, c->Yv, c->mpad, c->d_order, k, c->H0, c->gq, m, c->q, c->d, c->ab, c->tlwork, c->mem,
                        nullptr, nullptr, c->st, c->f32c));
  }
  double step = 0.0;
  const double* step_dev = nullptr;
  if (c->ss_type == 1 && c->has_L) {
    step = jl_min_h(1 / c->L, 1.0);
  } else if (c->ss_type == 1 && !c->has_L) {
    step = 0.5;
  } else if (c->ss_type == 2 || !c->has_L) {
    if (iter == 1) {
      step = 1.0;
    } else {
      grad_q_dev(c, xph, c->xp, c->gqn);  // ∇q(x_prev)
      HCK(launch_bb_step(c->x, c->xp, c->gq, c->gqn, m, c->scal + 12, c->st));
      step_dev = c->scal + 12;
    }
  } else if (c->ss_type == 3) {
    step = line_search(c, xh, c->x, c->d);
  } else {
    fail(c, SCS_ERR_REF, "Please, choose ss_type in [1, 2, 3].");
  }
  const double Mg = get_Mg(c, c->Mh, c->nu, c->mu, m);
  HCK(launch_score_tail(c->x, c->d, c->gr, c->Hr, m, c->lam, Mg, step, step_dev, prox_args(c), c->hinv, c->zb, c->xn,
                        c->dxv, c->scal, c->st));
  if (!c->dev_loop) {
    d2h(c, x_new, c->xn, m);
    if (dx) d2h(c, dx, c->dxv, m);
    d2h(c, c->hscal, c->scal, 4);
    sync(c);
    *pri = c->hscal[0];
  }
  // δh = x_new − x (prox) | dx (into q / dxv: grad_q_dev's smoother scratch is zb, hinv);
  // ∇q_new = grad_f(x_new) + λ gr(x_new)
  const double* dh = c->dxv;
  if (c->use_prox) {
    HCK(launch_sub(c->xn, c->x, m, c->q, c->st));
    dh = c->q;
  }
  grad_q_dev(c, x_new, c->xn, c->gqn);
  const int slot = c->spare;
  HCK(launch_lbfgs_update(dh, c->gqn, c->gq, m, c->S + (int64_t)slot * c->mpad, c->Yv + (int64_t)slot * c->mpad,
                          c->scal + 16, c->scal + 64, c->st));
  c->lbfgs_pending = true;
  c->lbfgs_slot = slot;
  if (!c->dev_loop) lbfgs_settle(c, false);
}

}  // namespace

namespace {
bool is_group(const scs_ctx* c);
template <class F>
int group_run(scs_ctx* g, F&& f);
int group_destroy(scs_ctx* g);
int group_set_data(scs_ctx* g, int64_t N, int64_t m, const void* A, int in32, int64_t lda, const double* y,
                   int64_t Nglob, int64_t row0);
int group_gen_data(scs_ctx* g, const scs_synth* sp);
int group_get_data(scs_ctx* g, int64_t r0, int64_t nr, double* A, int64_t lda_out, double* y);
int group_set_test_data(scs_ctx* g, int64_t N, const void* A, int in32, int64_t lda, const double* y, int64_t Nglob,
                        int64_t row0);
int group_gen_test_data(scs_ctx* g, const scs_synth* sp);
int group_eval(scs_ctx* g, const double* x, double* out, int64_t nout, int (*fn)(scs_ctx*, const double*, double*));
int group_step(scs_ctx* g, const double* x, const double* x_prev, int64_t iter, const double* grad_fx, double* x_new,
               double* dx, double* pri);
int group_iterate(scs_ctx* g, const double* x0, const double* x_star, int64_t max_epoch, double x_tol, double f_tol,
                  int rel_kind, double* x_out, const scs_history* h, int64_t* n_hist, int64_t* epochs);
}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

// SCS_SEGV_TRACE=1: a fatal-signal handler that names the shared object and offset of every
// frame (dladdr), for faults outside this library's symbols (e.g. runtime teardown at exit).
// Diagnostics only; installed when the library is loaded.
static void scs_fatal_trace(int sig, siginfo_t* si, void*) {
  void* fr[48];
  const int n = backtrace(fr, 48);
  fprintf(stderr, "[scsopt] signal %d, fault address %p, %d frames:\n", sig, si ? si->si_addr : nullptr, n);
  for (int i = 0; i < n; ++i) {
    Dl_info d;
    if (dladdr(fr[i], &d) && d.dli_fname)
      fprintf(stderr, "  #%-2d %s +0x%lx %s\n", i, d.dli_fname, (unsigned long)((char*)fr[i] - (char*)d.dli_fbase),
              d.dli_sname ? d.dli_sname : "");
    else
      fprintf(stderr, "  #%-2d %p\n", i, fr[i]);
  }
  fflush(stderr);
  signal(sig, SIG_DFL);
  raise(sig);
}

__attribute__((constructor)) static void scs_install_trace() {
  const char* e = getenv("SCS_SEGV_TRACE");
  if (!e || e[0] != '1') return;
  void* warm[2];
  (void)backtrace(warm, 2);   // loads the unwinder now, not inside the handler
  struct sigaction sa;
  memset(&sa, 0, sizeof(sa));
  sa.sa_sigaction = scs_fatal_trace;
  sa.sa_flags = SA_SIGINFO;
  sigaction(SIGSEGV, &sa, nullptr);
  sigaction(SIGBUS, &sa, nullptr);
  sigaction(SIGABRT, &sa, nullptr);
}

const char* scs_version(void) { return "libscsopt 0.1.0 (gfx950)"; }

int scs_create(int device, void* stream, scs_ctx** out) {
  if (!out) return SCS_ERR_ARG;
  *out = nullptr;
  scs_ctx* c = new scs_ctx();
  int rc = guarded(c, [&] {
    HCK(hipSetDevice(device));
    c->dev = device;
    if (stream) {
      c->st = (hipStream_t)stream;
    } else {
      HCK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
      c->own_stream = true;
    }
  });
  if (rc != SCS_OK) {
    delete c;
    return rc;
  }
  *out = c;
  return SCS_OK;
}

int scs_destroy(scs_ctx* c) {
  if (is_group(c)) return group_destroy(c);
  if (!c) return SCS_OK;
  (void)hipSetDevice(c->dev);
  (void)hipStreamSynchronize(c->st);
  for (auto& p : c->pending) {
    (void)hipEventDestroy(p.e0);
    (void)hipEventDestroy(p.e1);
  }
  if (c->rccl) (void)ncclCommDestroy(c->rccl);
  for (auto& a : c->allocs) (void)hipFree(a.p);
  if (c->hscal) (void)hipHostFree(c->hscal);
  if (c->hserr) (void)hipHostFree(c->hserr);
  if (c->hring) (void)hipHostFree(c->hring);
  if (c->hloop) (void)hipHostFree(c->hloop);
  for (hipEvent_t e : c->loop_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->cbh) (void)hipHostFree(c->cbh);
  if (c->swh) (void)hipHostFree(c->swh);
  for (auto& e : c->swy)
    if (e.h) (void)hipHostFree(e.h);
  lu_aux_free(&c->lu);
  qr_aux_free(&c->qr);
  qr_aux_free(&c->qre);
  chol_aux_free(&c->ceaux);
  if (c->sf) {
    (void)hipStreamSynchronize(c->sf);
    (void)hipStreamDestroy(c->sf);
  }
  for (hipEvent_t e : c->evstrip) (void)hipEventDestroy(e);
  if (c->evfac) (void)hipEventDestroy(c->evfac);
  if (c->own_stream) (void)hipStreamDestroy(c->st);
  delete c;
  return SCS_OK;
}

const char* scs_last_error(const scs_ctx* c) { return c ? c->err.c_str() : "null context"; }

int scs_get_stream(scs_ctx* c, void** stream) {
  if (is_group(c)) return (*stream = (void*)c->st), SCS_OK;
  return guarded(c, [&] { *stream = (void*)c->st; });
}

int scs_set_comm(scs_ctx* c, int rank, int nranks, scs_allreduce_fn fn, void* user) {
  return guarded(c, [&] {
    if (nranks < 1 || rank < 0 || rank >= nranks) fail(c, SCS_ERR_ARG, "bad rank/nranks %d/%d", rank, nranks);
    if (nranks > 1 && !fn) fail(c, SCS_ERR_ARG, "nranks > 1 needs an all-reduce callback");
    if (nranks > 1 && multi(c))
      fail(c, SCS_ERR_ARG, "nranks > 1 is not supported with scs_set_outputs (nout = %d)", c->nout);
    if (c->rccl) {
      (void)ncclCommDestroy(c->rccl);
      c->rccl = nullptr;
    }
    c->rank = rank;
    c->nranks = nranks;
    c->ar = fn;
    c->ar_user = user;
  });
}

int scs_rccl_unique_id(void* id) {
  if (!id) return SCS_ERR_ARG;
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return SCS_ERR_COMM;
  std::memcpy(id, &u, sizeof(u));
  return SCS_OK;
}

int scs_set_comm_rccl(scs_ctx* c, int rank, int nranks, const void* id) {
  return guarded(c, [&] {
    if (nranks < 1 || rank < 0 || rank >= nranks || !id)
      fail(c, SCS_ERR_ARG, "bad rank/nranks %d/%d or null id", rank, nranks);
    if (nranks > 1 && multi(c))
      fail(c, SCS_ERR_ARG, "nranks > 1 is not supported with scs_set_outputs (nout = %d)", c->nout);
    HCK(hipSetDevice(c->dev));
    sync(c);
    if (c->rccl) {
      (void)ncclCommDestroy(c->rccl);
      c->rccl = nullptr;
    }
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = ncclCommInitRank(&comm, nranks, u, rank);   // collective over the ranks
    if (r != ncclSuccess) fail(c, SCS_ERR_COMM, "ncclCommInitRank(%d of %d): %s", rank, nranks, ncclGetErrorString(r));
    c->rccl = comm;
    c->rank = rank;
    c->nranks = nranks;
    c->ar = nullptr;
    c->ar_user = nullptr;
  });
}

int scs_set_comm_force(scs_ctx* c, int on) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_comm_force(s_, on); });
  return guarded(c, [&] {
    if (on && !c->rccl && !c->ar) fail(c, SCS_ERR_STATE, "scs_set_comm_force needs a communicator");
    c->comm_force = on != 0;
  });
}

int scs_reduce_buffer_size(scs_ctx* c, int64_t* nd) {
  return guarded(c, [&] {
    if (!c->has_data) fail(c, SCS_ERR_STATE, "reduce buffer size needs the data dimensions");
    *nd = reduce_buffer_doubles(c);
  });
}

int scs_set_reduce_buffer(scs_ctx* c, void* p, int64_t nd) {
  return guarded(c, [&] {
    if (c->own_red) {
      dfree_t(c, c->red);
      c->own_red = false;
    }
    c->red = (double*)p;
    c->red_cap = nd;
  });
}

// the doors and kernel-level entry points that do not serve a multi-output context
static void refuse_multi(scs_ctx* c, const char* what) {
  if (multi(c)) fail(c, SCS_ERR_ARG, "%s is not supported with scs_set_outputs (nout = %d)", what, c->nout);
}

// a sparse door on a multi-output context: accepted in the scs_set_sparse_outputs mode (one rank)
static void refuse_multi_sparse(scs_ctx* c, const char* what, int64_t N, int64_t Nglob, int64_t row0) {
  if (!multi(c)) return;
  if (!c->sparse_outputs)
    fail(c, SCS_ERR_ARG, "%s is not supported with scs_set_outputs (nout = %d); pass sparse_outputs=True / "
                         "scs_set_sparse_outputs", what, c->nout);
  if (c->nranks > 1 || (Nglob > 0 && Nglob != N) || row0 != 0)
    fail(c, SCS_ERR_ARG, "scs_set_outputs (nout = %d) runs on one rank: nranks > 1 / a row shard is not supported",
         c->nout);
  if (c->f32c)
    fail(c, SCS_ERR_ARG, "scs_set_compute_f32 (the fp32-arithmetic products have one right-hand side) is not "
                         "supported with scs_set_outputs (nout = %d)", c->nout);
}

// Which arm forms the products of a sparse A with K right-hand sides: 1 the one-pass kernel
// (multi_sparse.hip), 0 K launches of the single-vector product.  SCS_MULTI_SPARSE_KERNEL=0 / 1 forces
// an arm (read at the data door); the default is the measured one per K and storage type
// (multi_spmm_default in multi_sparse.hip, the one place of the rule; DESIGN §2i, products table).
static int multi_sparse_arm(int K, int f32) {
  if (const char* e = std::getenv("SCS_MULTI_SPARSE_KERNEL")) return e[0] != '0';
  return multi_spmm_default(K, f32);
}

// The gather of a multi-output context's batches (scs_set_multi_batches): 1 multi.hip's one-launch kernel,
// 0 gather_rows_kernel over dcp columns plus launch_gather_y per further target column.  Both write the
// same bits.  SCS_MULTI_GATHER=0 / 1 forces an arm (read where the list is registered); the default is
// the measured one per storage type (multi_gather_default in multi.hip, the one place of the rule;
// DESIGN §2k).
static int multi_gather_arm(int a32) {
  if (const char* e = std::getenv("SCS_MULTI_GATHER")) return e[0] != '0';
  return multi_gather_default(a32);
}

// The workgroup form of the one-pass K-column kernel on sparse batch views (scs_set_multi_sparse_batches):
// 1 the 256-row form, 0 the 1024-row form.  Both write the same bits.  SCS_MULTI_SPARSE_NARROW=0 / 1
// forces a form (read where the list is registered); the default is multi_spmm_narrow_default in
// multi_sparse.hip, the one place of the rule.
static int multi_narrow_form(int K, int f32) {
  if (const char* e = std::getenv("SCS_MULTI_SPARSE_NARROW")) return e[0] != '0';
  return multi_spmm_narrow_default(K, f32);
}

static void set_dims(scs_ctx* c, int64_t N, int64_t m, int64_t Nglob, int64_t row0) {
  if (m <= 0 || N < 0) fail(c, SCS_ERR_ARG, "bad dimensions N=%lld m=%lld", (long long)N, (long long)m);
  c->N = N;
  c->dc = m;   // the data view's columns; the variable count is dc·K with scs_set_outputs
  c->dcp = round_up(m, 128);
  c->m = m * kout(c);
  c->Npad = std::max<int64_t>(round_up(std::max<int64_t>(N, 1), 16), 16);
  c->mpad = round_up(c->m, 128);
  c->nstage = c->Npad / 16;
  c->Nglob = Nglob > 0 ? Nglob : N;
  c->Nglob_data = c->Nglob;
  c->row0 = row0;
}

static void reset_data(scs_ctx* c) {
  if (c->own_red) {   // sized by the old dimensions
    dfree_t(c, c->red);
    c->red_cap = 0;
    c->own_red = false;
  }
  // the view in place: its buffers and fields (a32: the block's type goes with it; the mode, dense_f32,
  // persists, as the solver choice does)
  free_buffers(c, *c, VB_ALL);
  static_cast<ViewData&>(*c) = ViewData();
  if (c->prod_kname == GEMV_N_F32_NAME) c->prod_kname.clear();
  dfree_t(c, c->colptr);
  dfree_t(c, c->rowidx);
  dfree(c, c->valT);
  free_blk(c, c->bgram);
  dfree_t(c, c->sgseg.seg);
  dfree_t(c, c->sgseg.T);
  dfree_t(c, c->sgseg.tptr);
  dfree_t(c, c->sgseg.sw);
  c->sgseg.state = 0;
  dfree_t(c, c->Ad);
  dfree_t(c, c->ringA);
  c->sp_mode = 0;
  c->sp_gram = 0;
  c->ring_rows = 0;
  c->ring_r0[0] = c->ring_r0[1] = -1;
  dfree_t(c, c->Gk);
  dfree_t(c, c->Gd);
  dfree_t(c, c->mVt);
  c->mVt_cap = 0;
  free_view(c, c->cbv);
  dfree_t(c, c->cbstage);
  ++c->data_gen;
  dfree_t(c, c->G);
  dfree_t(c, c->Gc);
  dfree_t(c, c->tiles);
  dfree_t(c, c->utiles);
  dfree_t(c, c->gwork);
  dfree_t(c, c->gcomb);
  dfree_t(c, c->ptiles);
  dfree_t(c, c->pwork);
  dfree_t(c, c->pcomb);
  c->nptiles = c->pseglen = c->pncomb = 0;
  c->pnsplit = 1;
  dfree_t(c, c->gpart);
  dfree_t(c, c->vpart);
  for (auto& g : c->gstrip) {
    dfree_t(c, g.work);
    dfree_t(c, g.comb);
  }
  c->gstrip.clear();
  c->vpieces = 1;
  c->gseglen = c->gncomb = 0;
  c->gnsplit = 1;
  dfree_t(c, c->W);
  dfree_t(c, c->ysol);
  dfree_t(c, c->trilist);
  dfree_t(c, c->cinfo);
  dfree_t(c, c->lsbuf);
  c->lscap = 0;
  chol_aux_free(&c->caux);
  clear_batches(c);
  free_view(c, c->gview);
  free_test(c);
  c->gview_ok = false;
  c->ntiles = c->nslots = 0;
  invalidate_caches(c);
  c->has_data = false;
  c->reg_set = c->smooth_set = c->method_set = false;
}

// fp32 storage does not cover the quadratic loss (its m x m A goes through launch_half_sym)
static void refuse_f32_quadratic(scs_ctx* c, int a32) {
  if (a32 && c->loss_set && c->loss == SCS_LOSS_QUADRATIC)
    fail(c, SCS_ERR_ARG, "the quadratic loss needs an fp64-stored A: fp32 storage (scs_set_dense_f32 / "
                         "scs_set_data_f32) does not cover it");
}

// Where the rows of a dense block come from.  Host (dev = 0): column-major rows with leading
// dimension lda, in32: float elements.  Device (dev = 1, scs_set_data_device): element (n, j) at
// A[n*sn + j*sm], in32 likewise; src_stream: the producer's stream, or NULL.
struct DenseSrc {
  const void* A;
  int in32;
  int64_t lda;
  int dev = 0;
  int64_t sn = 0, sm = 0;
  hipStream_t src_stream = nullptr;
  int elem_bytes = 0;           // as the caller gave it (checked before in32 means anything)
  const char* what = nullptr;   // the entry point, for messages
};

// hipPointerGetAttributes on plain host memory: "unregistered" on current runtimes, an error (left
// in the thread's last-error slot, cleared here) on older ones
static bool is_device_ptr(const void* p, int* dev_out) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) return false;
  if (dev_out) *dev_out = at.device;
  return true;
}

static int refuse_group_device(scs_ctx* g, const char* what) {
  set_err(g, "%s takes a single-device context (scs_create): a multi-device context would have to split the "
             "device array across its devices", what);
  return SCS_ERR_ARG;
}

// the refusals of a device source, all before anything is queued or freed; `what` names the entry
static void check_device_src(scs_ctx* c, const DenseSrc& s, int64_t N, int64_t m) {
  const char* what = s.what;
  const int elem_bytes = s.elem_bytes;
  if (elem_bytes != 4 && elem_bytes != 8)
    fail(c, SCS_ERR_ARG, "%s: elem_bytes = %d (8: double, 4: float)", what, elem_bytes);
  if (N < 0 || m <= 0) fail(c, SCS_ERR_ARG, "%s: bad dimensions N=%lld m=%lld", what, (long long)N, (long long)m);
  if (s.sn != 1 && s.sm != 1)
    fail(c, SCS_ERR_ARG, "%s: both strides are non-unit (%lld, %lld): one of stride_n, stride_m must be 1 "
                         "(make the array contiguous)", what, (long long)s.sn, (long long)s.sm);
  const bool rows = s.sm == 1 && (s.sn != 1 || N <= 1);   // launch_tile_device's choice of layout
  if (rows ? (N > 1 && s.sn < m) : (m > 1 && s.sm < N))
    fail(c, SCS_ERR_ARG, "%s: stride_%s = %lld is smaller than the extent it spans (%lld)", what, rows ? "n" : "m",
         (long long)(rows ? s.sn : s.sm), (long long)(rows ? m : N));
  if (!s.A) fail(c, SCS_ERR_ARG, "%s: dA is NULL", what);
  if (N == 0) return;
  int dev = -1;
  if (!is_device_ptr(s.A, &dev))
    fail(c, SCS_ERR_ARG, "%s: dA is not device memory (hipPointerGetAttributes); host rows go through "
                         "scs_set_data", what);
  if (dev != c->dev)
    fail(c, SCS_ERR_ARG, "%s: dA lives on device %d, the context on device %d", what, dev, c->dev);
  // the matrix must lie inside its allocation (where the runtime can tell)
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)s.A) == hipSuccess) {
    const int64_t last = rows ? (N - 1) * s.sn + (m - 1) : (m - 1) * s.sm + (N - 1);
    const char* end = (const char*)s.A + (size_t)(last + 1) * elem_bytes;
    if (end > (const char*)base + size)
      fail(c, SCS_ERR_ARG, "%s: the strided matrix runs past the end of dA's allocation", what);
  } else {
    (void)hipGetLastError();
  }
}

// The context's stream waits for the work queued so far on the producer's stream of a device source
// (the dense and the sparse device door).
static void join_src_stream(scs_ctx* c, hipStream_t src_stream) {
  // __cuda_array_interface__'s two small integers are no handles, and a runtime that does not know
  // hipStreamLegacy reads (hipStream_t)1 as an object: neither value ever reaches the runtime as one.
  // 1, the legacy default stream, is the NULL stream; 2, the caller's per-thread default stream, is
  // covered by a device-wide synchronise.
  const uintptr_t sv = (uintptr_t)src_stream;
  if (sv == 2) {
    HCK(hipDeviceSynchronize());
  } else if (sv) {   // the work queued on the producer's stream so far
    hipEvent_t ev;
    HCK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, sv == 1 ? (hipStream_t) nullptr : src_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->st, ev, 0);
    (void)hipEventDestroy(ev);
    HCK(e);
  }
}

// y of a device door: a host or a device pointer (the library asks the pointer's attributes)
// (multi-output: N x K column-major with leading dimension N -> the view's stride Npad)
static void copy_y_any(scs_ctx* c, ViewData& v, const double* y, int64_t N) {
  if (!y || N <= 0) return;
  const bool ydev = is_device_ptr(y, nullptr);
  const hipMemcpyKind kind = ydev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (multi(c))
    HCK(hipMemcpy2DAsync(v.y, sizeof(double) * v.Npad, y, sizeof(double) * N, sizeof(double) * N, c->nout, kind,
                         c->st));
  else
    HCK(hipMemcpyAsync(v.y, y, sizeof(double) * N, kind, c->st));
}

// y of a host door (multi-output: N x nout, column-major)
static void upload_y(scs_ctx* c, ViewData& v, const double* y, int64_t N) {
  if (!y || N <= 0) return;
  if (multi(c)) {
    copy_y_any(c, v, y, N);
    sync(c);   // a pageable host source: the call returns with the copy done
  } else {
    h2d(c, v.y, y, N);
  }
}

// N rows of src -> the A and y of v (the data in place, or a view being built).  Host rows: panel by
// panel through the column-major staging buffer.  Device rows: one re-tile pass that writes the whole
// block, padding included.  Ends with the stream drained: the caller may free the source.
static void load_dense(scs_ctx* c, ViewData& v, const DenseSrc& s, int64_t N, const double* y) {
  if (s.dev) {
    join_src_stream(c, s.src_stream);
    HCK(launch_tile_device(s.A, s.in32, s.sn, s.sm, N, c->dc, v.Npad, c->dcp, v.A, v.a32, c->st));
    copy_y_any(c, v, y, N);
    sync(c);
    return;
  }
  if (N <= 0) return;
  double* C = dalloc<double>(c, (size_t)v.Npad * (s.in32 ? 64 : 128));   // Npad x 128 elements
  upload_panels(c, s.A, s.in32, N, s.lda, v.Npad, v.A, v.a32, C);
  sync(c);
  dfree_t(c, C);
  upload_y(c, v, y, N);
}

// scs_set_data (in32 = 0) / scs_set_data_f32 (in32 = 1: host floats, stored as they are) /
// scs_set_data_device (src.dev: the mode alone decides the stored type)
static int set_data_any(scs_ctx* c, int64_t N, int64_t m, const DenseSrc& src, const double* y, int64_t Nglob,
                        int64_t row0) {
  const void* A = src.A;
  const int in32 = src.dev ? 0 : src.in32;   // a host fp32 source switches the mode on
  if (is_group(c)) {
    if (src.dev) return refuse_group_device(c, src.what);
    return group_set_data(c, N, m, A, in32, src.lda, y, Nglob, row0);
  }
  return guarded(c, [&] {
    HCK(hipSetDevice(c->dev));
    if (multi(c)) {
      if (!A) fail(c, SCS_ERR_ARG, "scs_set_outputs (nout = %d) needs a dense A: a ProblemGeneric (A = NULL) has no outputs",
                   c->nout);
      if (c->nranks > 1 || (Nglob > 0 && Nglob != N) || row0 != 0)
        fail(c, SCS_ERR_ARG, "scs_set_outputs (nout = %d) runs on one rank: nranks > 1 / a row shard is not supported",
             c->nout);
    }
    if (src.dev) check_device_src(c, src, N, m);
    if (A) refuse_f32_quadratic(c, in32 | c->dense_f32);
    if (in32 && A) c->dense_f32 = 1;
    reset_data(c);
    set_dims(c, N, m, Nglob, row0);
    c->generic = (A == nullptr);
    if (!c->generic) {
      if (!src.dev && src.lda < N) fail(c, SCS_ERR_ARG, "lda (%lld) < N (%lld)", (long long)src.lda, (long long)N);
      c->a32 = c->dense_f32;
      c->A = alloc_A(c, c->Npad, c->a32, !src.dev);
      c->y = dalloc<double>(c, c->Npad * kout(c));
      load_dense(c, *c, src, N, y);
    }
    alloc_mspace(c);
    alloc_nspace(c);
    sync(c);
    c->has_data = true;
  });
}

int scs_set_data(scs_ctx* c, int64_t N, int64_t m, const double* A, int64_t lda, const double* y, int64_t Nglob,
                 int64_t row0) {
  return set_data_any(c, N, m, DenseSrc{A, 0, lda}, y, Nglob, row0);
}

static DenseSrc device_src(const char* what, const void* dA, int elem_bytes, int64_t sn, int64_t sm, void* stream) {
  DenseSrc s{dA, elem_bytes == 4, 0};
  s.dev = 1;
  s.sn = sn;
  s.sm = sm;
  s.src_stream = (hipStream_t)stream;
  s.elem_bytes = elem_bytes;
  s.what = what;
  return s;
}

int scs_set_data_device(scs_ctx* c, int64_t N, int64_t m, const void* dA, int elem_bytes, int64_t stride_n,
                        int64_t stride_m, const double* y, void* src_stream, int64_t Nglob, int64_t row0) {
  if (!c) return SCS_ERR_ARG;
  return set_data_any(c, N, m, device_src("scs_set_data_device", dA, elem_bytes, stride_n, stride_m, src_stream), y,
                      Nglob, row0);
}

int scs_set_data_f32(scs_ctx* c, int64_t N, int64_t m, const void* A32, int64_t lda, const double* y, int64_t Nglob,
                     int64_t row0) {
  if (!A32) {
    c->err = "scs_set_data_f32: A32 is NULL (a ProblemGeneric goes through scs_set_data)";
    return SCS_ERR_ARG;
  }
  return set_data_any(c, N, m, DenseSrc{A32, 1, lda}, y, Nglob, row0);
}

int scs_set_dense_f32(scs_ctx* c, int on) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_dense_f32(s_, on); });
  return guarded(c, [&] { c->dense_f32 = on ? 1 : 0; });
}

int scs_set_sparse_batches(scs_ctx* c, int on) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_sparse_batches(s_, on); });
  return guarded(c, [&] {
    const int v = on ? 1 : 0;
    if (v == c->sparse_batches) return;
    HCK(hipSetDevice(c->dev));
    sync(c);
    c->sparse_batches = v;
    free_dense_views(c);   // the pooled views go, the registered list stays
    free_sparse_views(c);
    invalidate_caches(c);
    if (c->bsel >= 0) select_batch(c, c->bsel);
    sync(c);
  });
}

int scs_set_sparse_sample(scs_ctx* c, int on) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_sparse_sample(s_, on); });
  return guarded(c, [&] {
    const int v = on ? 1 : 0;
    if (v == c->sparse_sample) return;
    HCK(hipSetDevice(c->dev));
    sync(c);
    c->sparse_sample = v;
    // the views follow the mode (the registered list stays); the other mode's sample-space scratch goes
    free_dense_views(c);
    free_sparse_views(c);
    free_sample_sys(c);
    if (c->sparse) {
      free_buffers(c, *c, VB_SAMPLE);
      dfree_t(c, c->Ad);
      c->nstiles = 0;
    }
    invalidate_caches(c);
    if (c->method_set) c->vkind = batch_view_kind(c, c->method);
    if (c->bsel >= 0) select_batch(c, c->bsel);
    sync(c);
  });
}

int scs_batch_info(scs_ctx* c, int64_t* nviews, int64_t* view_bytes, int64_t* builds) {
  if (is_group(c)) {   // the devices' figures summed
    int64_t nv = 0, vb = 0, bd = 0;
    for (scs_ctx* s_ : c->subs) {
      int64_t a = 0, b = 0, d = 0;
      const int rc = scs_batch_info(s_, &a, &b, &d);
      if (rc != SCS_OK) {
        c->err = s_->err;
        return rc;
      }
      nv += a;
      vb += b;
      bd += d;
    }
    if (nviews) *nviews = nv;
    if (view_bytes) *view_bytes = vb;
    if (builds) *builds = bd;
    return SCS_OK;
  }
  return guarded(c, [&] {
    int64_t nv = 0, vb = c->bplan.total_bytes();
    for (const scs::BatchSlot& s_ : c->bplan.slots) nv += s_.batch >= 0 ? 1 : 0;
    if (multi(c) && c->sparse)   // scs_set_multi_sparse_batches: the densified pool views count too
      for (size_t i = 0; i < c->bpool.size(); ++i) {
        if (c->bheld[i] < 0) continue;
        ++nv;
        size_t t = 0;
        view_buffers(c->bpool[i], VB_ALL, [&](const void* q) { t += alloc_bytes(c, q); });
        vb += (int64_t)t;
      }
    if (nviews) *nviews = nv;
    if (view_bytes) *view_bytes = vb;
    if (builds) *builds = c->bplan.builds;
  });
}

int scs_data_info(scs_ctx* c, int* a_elem_bytes, int64_t* a_bytes, int64_t* ctx_bytes) {
  if (is_group(c)) {   // device 0's element size, the devices' bytes summed
    int64_t ab = 0, cb = 0;
    for (size_t i = 0; i < c->subs.size(); ++i) {
      int64_t a1 = 0, c1 = 0;
      const int rc = scs_data_info(c->subs[i], i == 0 ? a_elem_bytes : nullptr, &a1, &c1);
      if (rc != SCS_OK) {
        c->err = c->subs[i]->err;
        return rc;
      }
      ab += a1;
      cb += c1;
    }
    if (a_bytes) *a_bytes = ab;
    if (ctx_bytes) *ctx_bytes = cb;
    return SCS_OK;
  }
  return guarded(c, [&] {
    const bool dense = c->has_data && !c->generic && !c->sparse && c->A;
    if (a_elem_bytes) *a_elem_bytes = (dense && c->a32) ? 4 : 8;
    if (a_bytes) *a_bytes = dense ? (int64_t)a_block_bytes(c, c->Npad, c->a32) : 0;
    if (ctx_bytes) {
      size_t t = 0;
      for (const DevBuf& b : c->allocs) t += b.bytes;
      *ctx_bytes = (int64_t)t;
    }
  });
}

int scs_gen_data(scs_ctx* c, const scs_synth* s) {
  if (is_group(c)) return group_gen_data(c, s);
  return guarded(c, [&] {
    if (!s) fail(c, SCS_ERR_ARG, "null synth spec");
    refuse_multi(c, "scs_gen_data (the synthetic generator has one target column)");
    HCK(hipSetDevice(c->dev));
    refuse_f32_quadratic(c, c->dense_f32);
    reset_data(c);
    set_dims(c, s->N, s->m, s->N_global, s->row0);
    c->generic = false;
    c->a32 = c->dense_f32;
    c->A = alloc_A(c, c->Npad, c->a32);
    c->y = dalloc<double>(c, c->Npad);
    alloc_mspace(c);
    alloc_nspace(c);
    const double scale = (s->kind == 3) ? 1.0 : 1.0 / std::sqrt((double)s->m);
    // fp32 mode: the rows are rounded as they are written, and y comes from the stored (rounded) rows
    HCK(launch_gen_A(c->A, c->a32, c->Npad, c->N, c->m, c->mpad, c->row0, s->seed, scale, c->st));
    HCK(launch_gen_xtrue(c->xn, c->m, s->seed, s->density, c->st));
    HCK(launch_gemv_n(c->A, c->a32, c->nstage, c->Npad, c->mpad, c->xn, 1, c->zpart, c->Npad, c->st));
    HCK(launch_gen_y(s->kind, c->zpart, c->y, c->N, c->row0, s->seed, c->st));
    sync(c);
    c->has_data = true;
  });
}

// rows [r0, r0 + nr) of the dense view in place (the full data, or a batch view inside a BatchScope) to
// the host: A column-major with leading dimension lda_out, y with nr rows (x nout, column-major)
static void read_rows(scs_ctx* c, int64_t r0, int64_t nr, double* A, int64_t lda_out, double* y) {
  if (A && nr > 0) {
    double* C = dalloc<double>(c, (size_t)c->Npad * 128);
    for (int64_t p = 0; p < c->dcp / 128; ++p) {
      const int64_t j0 = p * 128, nc = std::min<int64_t>(128, c->dc - j0);
      if (nc <= 0) break;
      HCK(launch_retile(C, 0, c->A, c->a32, c->Npad, p, 0, c->st));   // fp32-stored rows come back widened
      HCK(hipMemcpy2DAsync(A + j0 * lda_out, sizeof(double) * lda_out, C + r0, sizeof(double) * c->Npad,
                           sizeof(double) * nr, nc, hipMemcpyDeviceToHost, c->st));
    }
    sync(c);
    dfree_t(c, C);
  }
  if (y && nr > 0 && multi(c))   // nr x nout, column-major with leading dimension nr
    HCK(hipMemcpy2DAsync(y, sizeof(double) * nr, c->y + r0, sizeof(double) * c->Npad, sizeof(double) * nr, c->nout,
                         hipMemcpyDeviceToHost, c->st));
  else if (y && nr > 0)
    d2h(c, y, c->y + r0, nr);
  sync(c);
}

int scs_get_data(scs_ctx* c, int64_t r0, int64_t nr, double* A, int64_t lda_out, double* y) {
  if (is_group(c)) return group_get_data(c, r0, nr, A, lda_out, y);
  return guarded(c, [&] {
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    if (c->sparse && A) fail(c, SCS_ERR_ARG, "sparse A: use scs_get_sparse");
    if (r0 < 0 || nr < 0 || r0 + nr > c->N) fail(c, SCS_ERR_ARG, "row range out of bounds");
    read_rows(c, r0, nr, A, lda_out, y);
  });
}

int scs_get_dims(scs_ctx* c, int64_t* N, int64_t* m, int64_t* Ng, int64_t* r0) {
  if (is_group(c)) {   // the group holds the whole problem
    if (N) *N = c->grpN;
    if (m) *m = c->grpm;
    if (Ng) *Ng = c->grpN;
    if (r0) *r0 = 0;
    return SCS_OK;
  }
  return guarded(c, [&] {
    if (N) *N = c->N;
    if (m) *m = c->dc;   // A's columns (the variable count of a multi-output context: scs_get_outputs)
    if (Ng) *Ng = c->Nglob;
    if (r0) *r0 = c->row0;
  });
}

static void* dalloc_vals(scs_ctx* c, int64_t n, int f32) {
  return f32 ? (void*)dalloc<float>(c, (size_t)n) : (void*)dalloc<double>(c, (size_t)n);
}

static void upload_vals(scs_ctx* c, void* dst, const double* src, int64_t n, int f32) {
  if (!f32) {
    HCK(hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
    sync(c);
    return;
  }
  std::vector<float> h((size_t)n);
  for (int64_t i = 0; i < n; ++i) h[i] = (float)src[i];
  HCK(hipMemcpyAsync(dst, h.data(), sizeof(float) * n, hipMemcpyHostToDevice, c->st));
  sync(c);
}

// Sort each row's entries by index (in place: the arrays are replaced by sorted
// copies) and build the LDS-blocked copy B (sparse.hip).
// kcols > 1: the K-column layout of multi_sparse.hip (finer blocks, the same slots and padding).
// The arrays hold nnz entries of the float (f32) or double type.
static void build_blocked(scs_ctx* c, int64_t nnz, int f32, int64_t nrows, int64_t ncols, int64_t* ptr, int*& idx,
                          void*& val, SpBlkT& B, int kcols = 1) {
  size_t tb = 0;
  if (nnz > 0 && nrows > 0) {
    int end_bit = 1;
    while ((int64_t(1) << end_bit) < ncols) ++end_bit;
    int* idx_s = dalloc<int>(c, nnz);
    void* val_s = dalloc_vals(c, nnz, f32);
    HCK(sort_segments(nullptr, &tb, idx, idx_s, val, val_s, f32, nnz, nrows, ptr, end_bit, c->st));
    void* tmp = dalloc<char>(c, tb);
    HCK(sort_segments(tmp, &tb, idx, idx_s, val, val_s, f32, nnz, nrows, ptr, end_bit, c->st));
    sync(c);
    dfree(c, tmp);
    dfree_t(c, idx);
    dfree(c, val);
    idx = idx_s;
    val = val_s;
  }
  B.shift = kcols > 1 ? multi_spmm_shift(ncols, kcols) : spmv_blk_shift(ncols);
  B.kp = kcols > 1 ? multi_spmm_group(kcols) : 1;
  B.nblk = (int)ceil_div(ncols, int64_t(1) << B.shift);
  const int64_t nk = (int64_t)B.nblk * nrows;
  int64_t* cnt = dalloc<int64_t>(c, nk + 1);
  int64_t* first = dalloc<int64_t>(c, nk + 1);
  B.ptr = dalloc<int64_t>(c, nk + 1);
  if (nrows > 0) {
    HCK(blk_count(ptr, idx, nrows, B.shift, cnt, first, c->st));
    // segments in whole slots of 4 (fp64) / 8 (fp32) entries (padding: index 16384 = the SpMV's
    // zero slot, value 0; launch_spmv_blk)
    HCK(blk_pad(cnt, nk, f32, c->st));
    tb = 0;
    HCK(blk_scan(nullptr, &tb, cnt, B.ptr, nk + 1, c->st));
    void* tmp = dalloc<char>(c, tb);
    HCK(blk_scan(tmp, &tb, cnt, B.ptr, nk + 1, c->st));
    int64_t nnzp = 0;
    HCK(hipMemcpyAsync(&nnzp, B.ptr + nk, sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
    sync(c);
    dfree(c, tmp);
    B.lidx = dalloc<uint16_t>(c, nnzp + 8);
    HCK(hipMemsetD16Async((hipDeviceptr_t)B.lidx, (unsigned short)spmv_pad_index(), (size_t)(nnzp + 8), c->st));
    B.val = dalloc_vals(c, nnzp + 8, f32);
    HCK(blk_scatter(ptr, idx, val, f32, nrows, B.shift, B.ptr, first, B.lidx, B.val, c->st));
    sync(c);
  } else {
    B.lidx = dalloc<uint16_t>(c, 4);
    B.val = dalloc_vals(c, 4, f32);
  }
  sync(c);
  dfree_t(c, cnt);
  dfree_t(c, first);
}

// The CSC copy from the row-sorted CSR (after build_blocked on it), for a source that brings none
// (scs_set_sparse_device): claim, scan, place (sparse.hip).  Columns come out in arrival order of
// their runs; the stable sort of build_blocked on the CSC copy makes the order the host door's.
static void transpose_csr(scs_ctx* c) {
  const int64_t N = c->N, m = c->dc, nnz = c->nnz;   // the data view's columns
  c->colptr = dalloc<int64_t>(c, m + 1);
  c->rowidx = dalloc<int>(c, nnz, false);
  c->valT = c->sp_f32 ? (void*)dalloc<float>(c, (size_t)nnz, false) : (void*)dalloc<double>(c, (size_t)nnz, false);
  if (nnz <= 0 || N <= 0) return;
  int64_t* cnt = dalloc<int64_t>(c, m + 1);
  uint32_t* rank = dalloc<uint32_t>(c, (size_t)nnz, false);   // nnz < 2^32 (check_sparse_src)
  HCK(csr_claim(c->rowptr, c->colidx, N, cnt, rank, c->st));
  size_t tb = 0;
  HCK(blk_scan(nullptr, &tb, cnt, c->colptr, m + 1, c->st));
  void* tmp = dalloc<char>(c, tb);
  HCK(blk_scan(tmp, &tb, cnt, c->colptr, m + 1, c->st));
  HCK(csr_place(c->rowptr, c->colidx, c->val, c->sp_f32, N, c->colptr, rank, c->rowidx, c->valT, c->st));
  sync(c);
  dfree(c, tmp);
  dfree_t(c, rank);
  dfree_t(c, cnt);
}

// what scs_set_sparse and scs_set_sparse_device share once rowptr / colidx / val (and, from the host,
// colptr / rowidx / valT) and y are in place
static void finish_sparse(scs_ctx* c, bool transpose) {
  c->ms_kernel = multi(c) ? multi_sparse_arm(c->nout, c->sp_f32) : 0;   // read once, here: one set of copies per context
  const int kc = c->ms_kernel ? c->nout : 1;
  build_blocked(c, c->nnz, c->sp_f32, c->N, c->dc, c->rowptr, c->colidx, c->val, c->bcsr, kc);
  if (transpose) transpose_csr(c);
  build_blocked(c, c->nnz, c->sp_f32, c->dc, c->N, c->colptr, c->rowidx, c->valT, c->bcsc, kc);
  alloc_mspace(c);
  alloc_nspace(c);
  sync(c);
  c->has_data = true;
}

// the held-out counterpart, on the held-out view with its CSR and y in place: the row copy only (the arm
// of a sparse A's context is the one its data door read), the workspace sized by the data's column copy
static void finish_sparse_test(scs_ctx* c) {
  NView& v = c->tset.v;
  const int arm = !multi(c) ? 0 : c->sparse ? c->ms_kernel : multi_sparse_arm(c->nout, v.sp_f32);
  build_blocked(c, v.nnz, v.sp_f32, v.N, c->dc, v.rowptr, v.colidx, v.val, v.bcsr, arm ? c->nout : 1);
  alloc_nspace(c, v, c->bcsc);
  sync(c);
  c->tset.on = true;
}

int scs_set_sparse(scs_ctx* c, int64_t N, int64_t m, int64_t nnz, const int64_t* rowptr, const int32_t* colidx,
                   const double* val, const int64_t* colptr, const int32_t* rowidx, const double* valT, int f32,
                   const double* y, int64_t Nglob, int64_t row0) {
  return guarded(c, [&] {
    refuse_multi_sparse(c, "a sparse A (scs_set_sparse)", N, Nglob, row0);
    if (nnz < 0 || !rowptr || !colptr || (nnz > 0 && (!colidx || !val || !rowidx || !valT)))
      fail(c, SCS_ERR_ARG, "sparse A: null arrays");
    if (rowptr[0] != 0 || rowptr[N] != nnz || colptr[0] != 0 || colptr[m] != nnz)
      fail(c, SCS_ERR_ARG, "sparse A: rowptr/colptr must start at 0 and end at nnz");
    for (int64_t i = 0; i < N; ++i)
      if (rowptr[i + 1] < rowptr[i]) fail(c, SCS_ERR_ARG, "sparse A: rowptr not monotone at %lld", (long long)i);
    for (int64_t j = 0; j < m; ++j)
      if (colptr[j + 1] < colptr[j]) fail(c, SCS_ERR_ARG, "sparse A: colptr not monotone at %lld", (long long)j);
    for (int64_t p = 0; p < nnz; ++p)
      if (colidx[p] < 0 || colidx[p] >= m || rowidx[p] < 0 || rowidx[p] >= N)
        fail(c, SCS_ERR_ARG, "sparse A: index out of range at %lld", (long long)p);
    if (nnz > INT32_MAX * 64LL) fail(c, SCS_ERR_ARG, "sparse A: nnz too large");
    HCK(hipSetDevice(c->dev));
    reset_data(c);
    set_dims(c, N, m, Nglob, row0);
    c->generic = false;
    c->sparse = true;
    c->sp_f32 = f32 ? 1 : 0;
    c->nnz = nnz;
    c->rowptr = dalloc<int64_t>(c, N + 1);
    c->colptr = dalloc<int64_t>(c, m + 1);
    c->colidx = dalloc<int>(c, nnz);
    c->rowidx = dalloc<int>(c, nnz);
    c->val = dalloc_vals(c, nnz, c->sp_f32);
    c->valT = dalloc_vals(c, nnz, c->sp_f32);
    HCK(hipMemcpyAsync(c->rowptr, rowptr, sizeof(int64_t) * (N + 1), hipMemcpyHostToDevice, c->st));
    HCK(hipMemcpyAsync(c->colptr, colptr, sizeof(int64_t) * (m + 1), hipMemcpyHostToDevice, c->st));
    if (nnz > 0) {
      HCK(hipMemcpyAsync(c->colidx, colidx, sizeof(int) * nnz, hipMemcpyHostToDevice, c->st));
      HCK(hipMemcpyAsync(c->rowidx, rowidx, sizeof(int) * nnz, hipMemcpyHostToDevice, c->st));
      upload_vals(c, c->val, val, nnz, c->sp_f32);
      upload_vals(c, c->valT, valT, nnz, c->sp_f32);
    }
    c->y = dalloc<double>(c, c->Npad * kout(c));
    upload_y(c, *c, y, N);
    finish_sparse(c, false);
  });
}

// ---- a CSR that is already on the device (scs_set_sparse_device / scs_set_test_sparse_device) -------
struct SparseSrc {
  const void* ptr;
  int ptr_bytes;
  const void* idx;
  int idx_bytes;
  const void* val;
  int val_bytes;
  hipStream_t src_stream;
  const char* what;   // the entry point, for messages
};

// one source array: device memory on the context's device, inside its allocation (where the runtime can tell)
static void check_device_array(scs_ctx* c, const char* what, const char* name, const void* p, int64_t n, int eb) {
  int dev = -1;
  if (!is_device_ptr(p, &dev))
    fail(c, SCS_ERR_ARG, "%s: %s is not device memory (hipPointerGetAttributes); host arrays go through "
                         "scs_set_sparse", what, name);
  if (dev != c->dev) fail(c, SCS_ERR_ARG, "%s: %s lives on device %d, the context on device %d", what, name, dev, c->dev);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess) {
    if ((const char*)p + (size_t)n * eb > (const char*)base + size)
      fail(c, SCS_ERR_ARG, "%s: %s (%lld entries of %d bytes) runs past the end of its allocation", what, name,
           (long long)n, eb);
  } else {
    (void)hipGetLastError();
  }
}

// the host-side refusals of a device CSR, all before anything is queued or freed
static void check_sparse_src(scs_ctx* c, const SparseSrc& s, int64_t N, int64_t m, int64_t nnz) {
  const char* what = s.what;
  if (s.ptr_bytes != 4 && s.ptr_bytes != 8)
    fail(c, SCS_ERR_ARG, "%s: ptr_bytes = %d (8: int64, 4: int32)", what, s.ptr_bytes);
  if (s.idx_bytes != 4 && s.idx_bytes != 8)
    fail(c, SCS_ERR_ARG, "%s: idx_bytes = %d (8: int64, 4: int32)", what, s.idx_bytes);
  if (s.val_bytes != 4 && s.val_bytes != 8)
    fail(c, SCS_ERR_ARG, "%s: val_bytes = %d (8: double, 4: float)", what, s.val_bytes);
  if (N < 0 || N > INT32_MAX || m <= 0 || m > INT32_MAX || nnz < 0)   // both index copies are int32
    fail(c, SCS_ERR_ARG, "%s: bad dimensions N=%lld m=%lld nnz=%lld", what, (long long)N, (long long)m, (long long)nnz);
  // the host door's limit is INT32_MAX * 64; the segmented sort both doors run counts its items in 32
  // unsigned bits, and this door does not hand it more
  if (nnz > (int64_t)UINT32_MAX)
    fail(c, SCS_ERR_ARG, "%s: nnz too large (%lld: the per-row and per-column sorts take at most 2^32 - 1 entries)",
         what, (long long)nnz);
  if (!s.ptr) fail(c, SCS_ERR_ARG, "%s: d_rowptr is NULL", what);
  if (nnz > 0 && !s.idx) fail(c, SCS_ERR_ARG, "%s: d_colidx is NULL with nnz = %lld", what, (long long)nnz);
  if (nnz > 0 && !s.val) fail(c, SCS_ERR_ARG, "%s: d_val is NULL with nnz = %lld", what, (long long)nnz);
  check_device_array(c, what, "d_rowptr", s.ptr, N + 1, s.ptr_bytes);
  if (nnz > 0) {
    check_device_array(c, what, "d_colidx", s.idx, nnz, s.idx_bytes);
    check_device_array(c, what, "d_val", s.val, nnz, s.val_bytes);
  }
}

// The source -> fresh rowptr (int64) / colidx (int32) / val (stored type) buffers, validated on the
// device in the same pass (sparse.hip csr_ingest) and read back as one small record.  The context
// itself is untouched: a refusal frees the buffers and leaves the earlier data usable.
struct CsrBufs {
  int64_t* rowptr = nullptr;
  int* colidx = nullptr;
  void* val = nullptr;
};

static CsrBufs ingest_csr(scs_ctx* c, const SparseSrc& s, int64_t N, int64_t m, int64_t nnz, int f32) {
  join_src_stream(c, s.src_stream);
  CsrBufs b;
  b.rowptr = dalloc<int64_t>(c, N + 1, false);
  b.colidx = dalloc<int>(c, nnz, false);
  b.val = f32 ? (void*)dalloc<float>(c, (size_t)nnz, false) : (void*)dalloc<double>(c, (size_t)nnz, false);
  unsigned long long* drec = dalloc<unsigned long long>(c, 2, false);
  unsigned long long rec[2] = {0, 0};
  HCK(hipMemsetAsync(drec, 0xFF, sizeof(rec), c->st));
  HCK(csr_ingest(s.ptr, s.ptr_bytes, s.idx, s.idx_bytes, s.val, s.val_bytes, N, m, nnz, b.rowptr, b.colidx, b.val,
                 f32, drec, c->st));
  HCK(hipMemcpyAsync(rec, drec, sizeof(rec), hipMemcpyDeviceToHost, c->st));
  sync(c);
  dfree_t(c, drec);
  if (rec[0] != ~0ull || rec[1] != ~0ull) {
    dfree_t(c, b.rowptr);
    dfree_t(c, b.colidx);
    dfree(c, b.val);
    if (rec[0] != ~0ull) {
      const long long row = (long long)(rec[0] >> 2);
      switch ((int)(rec[0] & 3)) {
        case 0: fail(c, SCS_ERR_ARG, "%s: rowptr must start at 0 (row %lld)", s.what, row);
        case 1: fail(c, SCS_ERR_ARG, "%s: rowptr not monotone at row %lld", s.what, row);
        default: fail(c, SCS_ERR_ARG, "%s: rowptr must end at nnz = %lld (row %lld)", s.what, (long long)nnz, row);
      }
    }
    fail(c, SCS_ERR_ARG, "%s: column index outside [0, %lld) at position %lld", s.what, (long long)m,
         (long long)rec[1]);
  }
  return b;
}

int scs_set_sparse_device(scs_ctx* c, int64_t N, int64_t m, int64_t nnz, const void* d_rowptr, int ptr_bytes,
                          const void* d_colidx, int idx_bytes, const void* d_val, int val_bytes, int f32,
                          const double* y, void* src_stream, int64_t Nglob, int64_t row0) {
  if (!c) return SCS_ERR_ARG;
  const SparseSrc s{d_rowptr, ptr_bytes, d_colidx, idx_bytes, d_val, val_bytes, (hipStream_t)src_stream,
                    "scs_set_sparse_device"};
  if (is_group(c)) return refuse_group_device(c, s.what);
  return guarded(c, [&] {
    refuse_multi_sparse(c, "a sparse A (scs_set_sparse_device)", N, Nglob, row0);
    HCK(hipSetDevice(c->dev));
    check_sparse_src(c, s, N, m, nnz);
    const CsrBufs b = ingest_csr(c, s, N, m, nnz, f32 ? 1 : 0);
    reset_data(c);
    set_dims(c, N, m, Nglob, row0);
    c->generic = false;
    c->sparse = true;
    c->sp_f32 = f32 ? 1 : 0;
    c->nnz = nnz;
    c->rowptr = b.rowptr;
    c->colidx = b.colidx;
    c->val = b.val;
    c->y = dalloc<double>(c, c->Npad * kout(c));
    copy_y_any(c, *c, y, N);
    finish_sparse(c, true);
  });
}

int scs_gen_sparse(scs_ctx* c, const scs_synth* s, int f32) {
  return guarded(c, [&] {
    if (!s) fail(c, SCS_ERR_ARG, "null synth spec");
    refuse_multi(c, "a sparse A (scs_gen_sparse)");
    if (s->kind != 4) fail(c, SCS_ERR_ARG, "scs_gen_sparse: kind must be 4");
    const int64_t N = s->N, m = s->m;
    if (N <= 0 || (N & (N - 1)) != 0 || m <= 0 || N % m != 0)
      fail(c, SCS_ERR_ARG, "scs_gen_sparse: N must be a power of two and a multiple of m");
    if ((s->N_global > 0 && s->N_global != N) || s->row0 != 0)
      fail(c, SCS_ERR_ARG, "scs_gen_sparse: single-context generator (shard with scs_set_sparse)");
    const int k = (int)std::max<int64_t>(1, std::llround(s->density * (double)m));
    if (k > m) fail(c, SCS_ERR_ARG, "scs_gen_sparse: density > 1");
    const int64_t nnz = N * (int64_t)k;
    HCK(hipSetDevice(c->dev));
    reset_data(c);
    set_dims(c, N, m, N, 0);
    c->generic = false;
    c->sparse = true;
    c->sp_f32 = f32 ? 1 : 0;
    c->nnz = nnz;
    c->rowptr = dalloc<int64_t>(c, N + 1);
    c->colptr = dalloc<int64_t>(c, m + 1);
    c->colidx = dalloc<int>(c, nnz);
    c->rowidx = dalloc<int>(c, nnz);
    c->val = dalloc_vals(c, nnz, c->sp_f32);
    c->valT = dalloc_vals(c, nnz, c->sp_f32);
    c->y = dalloc<double>(c, c->Npad);
    alloc_mspace(c);
    std::vector<char> maps(sparse_layer_map_bytes(k));
    sparse_layer_maps(s->seed, k, N, maps.data());
    void* dmaps = dalloc<char>(c, maps.size());
    HCK(hipMemcpyAsync(dmaps, maps.data(), maps.size(), hipMemcpyHostToDevice, c->st));
    HCK(launch_gen_sparse(N, m, k, s->seed, dmaps, c->sp_f32, 1.0 / std::sqrt((double)k), c->rowptr, c->colidx,
                          c->val, c->colptr, c->rowidx, c->valT, c->st));
    build_blocked(c, nnz, c->sp_f32, N, m, c->rowptr, c->colidx, c->val, c->bcsr);
    build_blocked(c, nnz, c->sp_f32, m, N, c->colptr, c->rowidx, c->valT, c->bcsc);
    alloc_nspace(c);
    HCK(launch_gen_uniform(c->xn, m, s->seed, -1.5, 1.5, c->st));
    const int ns = matvec_n(c, c->xn, c->nsplit);
    HCK(launch_epilogue(SCS_LOSS_LEAST_SQUARES, SCS_GGN_NONE, EPI_Z, c->zpart, ns, c->Npad, c->y, c->N, c->Npad, 1.0,
                        c->z, nullptr, nullptr, nullptr, nullptr, c->valpart, c->st));
    HCK(launch_gen_y(3, c->z, c->y, c->N, 0, s->seed, c->st));
    sync(c);
    dfree(c, dmaps);
    c->has_data = true;
  });
}

int scs_get_nnz(scs_ctx* c, int64_t* nnz) {
  return guarded(c, [&] {
    if (!c->has_data || !c->sparse) fail(c, SCS_ERR_STATE, "no sparse data");
    *nnz = c->nnz;
  });
}

// one compressed copy (nseg + 1 pointers, nnz indices and values) back to the host, values widened
static void get_compressed(scs_ctx* c, int64_t nseg, const int64_t* dptr, const int* didx, const void* dval,
                           int64_t* ptr, int32_t* idx, double* val) {
  if (!c->has_data || !c->sparse) fail(c, SCS_ERR_STATE, "no sparse data");
  if (ptr) HCK(hipMemcpyAsync(ptr, dptr, sizeof(int64_t) * (nseg + 1), hipMemcpyDeviceToHost, c->st));
  if (idx && c->nnz) HCK(hipMemcpyAsync(idx, didx, sizeof(int) * c->nnz, hipMemcpyDeviceToHost, c->st));
  if (val && c->nnz) {
    if (c->sp_f32) {
      std::vector<float> h((size_t)c->nnz);
      HCK(hipMemcpyAsync(h.data(), dval, sizeof(float) * c->nnz, hipMemcpyDeviceToHost, c->st));
      sync(c);
      for (int64_t p = 0; p < c->nnz; ++p) val[p] = h[p];
    } else {
      HCK(hipMemcpyAsync(val, dval, sizeof(double) * c->nnz, hipMemcpyDeviceToHost, c->st));
    }
  }
  sync(c);
}

int scs_get_sparse(scs_ctx* c, int64_t* rowptr, int32_t* colidx, double* val) {
  return guarded(c, [&] { get_compressed(c, c->N, c->rowptr, c->colidx, c->val, rowptr, colidx, val); });
}

int scs_get_sparse_csc(scs_ctx* c, int64_t* colptr, int32_t* rowidx, double* valT) {
  return guarded(c, [&] { get_compressed(c, c->dc, c->colptr, c->rowidx, c->valT, colptr, rowidx, valT); });
}

// ---- held-out data (Problem(...; Atest, ytest), problems.jl:27-28,67-68) -----------------------
// the rows of a new held-out view (after free_test): Npad, nstage and the buffers of its dense form
static void test_view_dims(scs_ctx* c, int64_t N, int64_t Nglob, bool sparse, bool zero_A = true) {
  if (!c->has_data || c->generic)
    fail(c, SCS_ERR_STATE, "test data needs a data problem: call scs_set_data / scs_gen_data / scs_set_sparse first");
  if (N < 0) fail(c, SCS_ERR_ARG, "test data: N = %lld", (long long)N);
  NView& v = c->tset.v;
  v.N = N;
  v.Nglob = Nglob > 0 ? Nglob : N;
  v.Npad = std::max<int64_t>(round_up(std::max<int64_t>(N, 1), 16), 16);
  v.nstage = v.Npad / 16;
  v.sparse = sparse;
  v.y = dalloc<double>(c, v.Npad * kout(c));
  if (!sparse) {   // dense held-out rows follow the context's storage mode
    v.a32 = c->dense_f32;
    v.A = alloc_A(c, v.Npad, v.a32, zero_A);
  }
}

// scs_set_test_data (in32 = 0) / scs_set_test_data_f32 (in32 = 1)
static int set_test_any(scs_ctx* c, int64_t N, const DenseSrc& src, const double* y, int64_t Nglob, int64_t row0) {
  const void* A = src.A;
  const int in32 = src.dev ? 0 : src.in32;
  const int64_t lda = src.dev ? N : src.lda;
  if (is_group(c)) {
    if (src.dev) return refuse_group_device(c, src.what);
    return group_set_test_data(c, N, A, in32, lda, y, Nglob, row0);
  }
  return guarded(c, [&] {
    HCK(hipSetDevice(c->dev));
    if (src.dev) {
      if (!y) fail(c, SCS_ERR_ARG, "%s: y is NULL (dA and y are both required)", src.what);
      if (!c->has_data || c->generic)
        fail(c, SCS_ERR_STATE, "test data needs a data problem: call scs_set_data / scs_gen_data / scs_set_sparse first");
      check_device_src(c, src, N, c->dc);
    }
    if (A && y) refuse_f32_quadratic(c, in32 | c->dense_f32);
    if (in32 && A) c->dense_f32 = 1;
    free_test(c);
    if (!A && !y) return;   // clears the held-out set
    if (!A || !y) {         // the reference's xor case (iterate.jl:170-171): recorded, not an error here
      c->tset.xor_case = true;
      return;
    }
    if (lda < N) fail(c, SCS_ERR_ARG, "test data: lda (%lld) < N (%lld)", (long long)lda, (long long)N);
    (void)row0;
    test_view_dims(c, N, Nglob, false, !src.dev);
    load_dense(c, c->tset.v, src, N, y);
    alloc_nspace(c, c->tset.v);
    sync(c);
    c->tset.on = true;
  });
}

int scs_set_test_data(scs_ctx* c, int64_t N, const double* A, int64_t lda, const double* y, int64_t Nglob,
                      int64_t row0) {
  return set_test_any(c, N, DenseSrc{A, 0, lda}, y, Nglob, row0);
}

int scs_set_test_data_device(scs_ctx* c, int64_t N, const void* dA, int elem_bytes, int64_t stride_n,
                             int64_t stride_m, const double* y, void* src_stream, int64_t Nglob, int64_t row0) {
  if (!c) return SCS_ERR_ARG;
  return set_test_any(c, N, device_src("scs_set_test_data_device", dA, elem_bytes, stride_n, stride_m, src_stream), y,
                      Nglob, row0);
}

int scs_set_test_data_f32(scs_ctx* c, int64_t N, const void* A32, int64_t lda, const double* y, int64_t Nglob,
                          int64_t row0) {
  return set_test_any(c, N, DenseSrc{A32, 1, lda}, y, Nglob, row0);
}

int scs_set_test_sparse(scs_ctx* c, int64_t N, int64_t nnz, const int64_t* rowptr, const int32_t* colidx,
                        const double* val, int f32, const double* y, int64_t Nglob, int64_t row0) {
  if (is_group(c)) {
    c->err = "sparse test data takes a single-device context";
    return SCS_ERR_ARG;
  }
  return guarded(c, [&] {
    refuse_multi_sparse(c, "sparse held-out rows (scs_set_test_sparse)", N, Nglob, 0);
    HCK(hipSetDevice(c->dev));
    free_test(c);
    if (!rowptr || !y || nnz < 0 || (nnz > 0 && (!colidx || !val)))
      fail(c, SCS_ERR_ARG, "sparse test data: null arrays (Atest and ytest are both required)");
    if (N < 0 || rowptr[0] != 0 || rowptr[N] != nnz)
      fail(c, SCS_ERR_ARG, "sparse test data: rowptr must start at 0 and end at nnz");
    for (int64_t i = 0; i < N; ++i)
      if (rowptr[i + 1] < rowptr[i]) fail(c, SCS_ERR_ARG, "sparse test data: rowptr not monotone at %lld", (long long)i);
    for (int64_t p = 0; p < nnz; ++p)
      if (colidx[p] < 0 || colidx[p] >= c->dc)
        fail(c, SCS_ERR_ARG, "sparse test data: column index out of range at %lld", (long long)p);
    if (nnz > INT32_MAX * 64LL) fail(c, SCS_ERR_ARG, "sparse test data: nnz too large");
    (void)row0;
    test_view_dims(c, N, Nglob, true);
    NView& v = c->tset.v;
    v.sp_f32 = f32 ? 1 : 0;
    v.nnz = nnz;
    v.rowptr = dalloc<int64_t>(c, N + 1);
    v.colidx = dalloc<int>(c, nnz);
    v.val = dalloc_vals(c, nnz, v.sp_f32);
    HCK(hipMemcpyAsync(v.rowptr, rowptr, sizeof(int64_t) * (N + 1), hipMemcpyHostToDevice, c->st));
    if (nnz > 0) {
      HCK(hipMemcpyAsync(v.colidx, colidx, sizeof(int) * nnz, hipMemcpyHostToDevice, c->st));
      upload_vals(c, v.val, val, nnz, v.sp_f32);
    }
    upload_y(c, v, y, N);
    finish_sparse_test(c);
  });
}

int scs_set_test_sparse_device(scs_ctx* c, int64_t N, int64_t nnz, const void* d_rowptr, int ptr_bytes,
                               const void* d_colidx, int idx_bytes, const void* d_val, int val_bytes, int f32,
                               const double* y, void* src_stream, int64_t Nglob, int64_t row0) {
  if (!c) return SCS_ERR_ARG;
  const SparseSrc s{d_rowptr, ptr_bytes, d_colidx, idx_bytes, d_val, val_bytes, (hipStream_t)src_stream,
                    "scs_set_test_sparse_device"};
  if (is_group(c)) return refuse_group_device(c, s.what);
  return guarded(c, [&] {
    refuse_multi_sparse(c, "sparse held-out rows (scs_set_test_sparse_device)", N, Nglob, 0);
    HCK(hipSetDevice(c->dev));
    if (!y) fail(c, SCS_ERR_ARG, "%s: y is NULL (the CSR arrays and y are both required)", s.what);
    if (!c->has_data || c->generic)
      fail(c, SCS_ERR_STATE, "test data needs a data problem: call scs_set_data / scs_gen_data / scs_set_sparse first");
    check_sparse_src(c, s, N, c->dc, nnz);
    const CsrBufs b = ingest_csr(c, s, N, c->dc, nnz, f32 ? 1 : 0);
    free_test(c);
    (void)row0;
    test_view_dims(c, N, Nglob, true);
    NView& v = c->tset.v;
    v.sp_f32 = f32 ? 1 : 0;
    v.nnz = nnz;
    v.rowptr = b.rowptr;
    v.colidx = b.colidx;
    v.val = b.val;
    copy_y_any(c, v, y, N);
    finish_sparse_test(c);
  });
}

int scs_gen_test_data(scs_ctx* c, const scs_synth* s) {
  if (is_group(c)) return group_gen_test_data(c, s);
  return guarded(c, [&] {
    if (!s) fail(c, SCS_ERR_ARG, "null synth spec");
    refuse_multi(c, "scs_gen_test_data (the synthetic generator has one target column)");
    if (s->kind < 1 || s->kind > 3) fail(c, SCS_ERR_ARG, "scs_gen_test_data: dense kinds 1-3");
    if (s->m != c->m) fail(c, SCS_ERR_ARG, "scs_gen_test_data: m = %lld, the data has %lld", (long long)s->m,
                           (long long)c->m);
    HCK(hipSetDevice(c->dev));
    refuse_f32_quadratic(c, c->dense_f32);
    free_test(c);
    test_view_dims(c, s->N, s->N_global, false);
    NView& v = c->tset.v;
    alloc_nspace(c, v);
    const double scale = (s->kind == 3) ? 1.0 : 1.0 / std::sqrt((double)s->m);
    // rows [row0, row0 + N) of the same generator as scs_gen_data: with row0 >= the data's N_global
    // they are held-out samples of the same distribution (the same x_true)
    HCK(launch_gen_A(v.A, v.a32, v.Npad, v.N, c->m, c->mpad, s->row0, s->seed, scale, c->st));
    HCK(launch_gen_xtrue(c->xn, c->m, s->seed, s->density, c->st));
    HCK(launch_gemv_n(v.A, v.a32, v.nstage, v.Npad, c->mpad, c->xn, 1, v.zpart, v.Npad, c->st));
    HCK(launch_gen_y(s->kind, v.zpart, v.y, v.N, s->row0, s->seed, c->st));
    sync(c);
    c->tset.on = true;
  });
}

int scs_set_test_callback(scs_ctx* c, int on) {
  if (is_group(c)) {
    c->err = "a callback loss takes a single-device context";
    return SCS_ERR_ARG;
  }
  return guarded(c, [&] {
    free_test(c);
    if (!on) return;
    if (c->loss != SCS_LOSS_CALLBACK || !c->cb)
      fail(c, SCS_ERR_STATE, "scs_set_test_callback: the loss is not a callback (scs_set_loss_callback first)");
    c->tset.on = c->tset.host = true;
  });
}

int scs_eval_ftest(scs_ctx* c, const double* x, double* fval) {
  if (is_group(c)) return group_eval(c, x, fval, 1, scs_eval_ftest);
  return guarded(c, [&] {
    if (!x || !fval) fail(c, SCS_ERR_ARG, "scs_eval_ftest: null argument");
    if (!c->has_data || !c->loss_set) fail(c, SCS_ERR_STATE, "scs_eval_ftest: needs the data and the loss");
    HCK(hipSetDevice(c->dev));
    h2d(c, c->xn, x, c->m);
    *fval = eval_ftest_dev(c, x, c->xn);
  });
}

int scs_has_test(scs_ctx* c, int* on) {
  if (!on) return SCS_ERR_ARG;
  if (is_group(c)) return scs_has_test(c->subs[0], on);
  *on = c->tset.on ? 1 : 0;
  return SCS_OK;
}

int scs_set_loss(scs_ctx* c, int loss, int ggn, double scale) {
  if (is_group(c) && (loss == SCS_LOSS_SAMPLEWISE || ggn == SCS_GGN_SAMPLEWISE)) {
    c->err = "a sample-wise loss takes a single-device context (a group's devices run one host thread each)";
    return SCS_ERR_ARG;
  }
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_loss(s_, loss, ggn, scale); });
  return guarded(c, [&] {
    if (loss < SCS_LOSS_LOGISTIC_MARGIN || loss > SCS_LOSS_MULTI_LS) fail(c, SCS_ERR_ARG, "unknown loss %d", loss);
    if (ggn < SCS_GGN_NONE || ggn > SCS_GGN_LINEAR_MULTI_LS) fail(c, SCS_ERR_ARG, "unknown ggn kind %d", ggn);
    if (multi(c) && !multi_loss(loss)) {
      const char* const names[] = {"", "logistic_margin", "logistic_ce", "least_squares", "quadratic", "rosenbrock",
                                   "callback", "samplewise"};
      fail(c, SCS_ERR_ARG, "scs_set_outputs (nout = %d) takes SCS_LOSS_SOFTMAX_CE or SCS_LOSS_MULTI_LS, not the %s loss "
                           "(kind %d)", c->nout, names[loss], loss);
    }
    if (multi_loss(loss) && !multi(c))
      fail(c, SCS_ERR_ARG, "SCS_LOSS_SOFTMAX_CE / SCS_LOSS_MULTI_LS need scs_set_outputs(nout) before the data");
    if ((ggn == SCS_GGN_LINEAR_SOFTMAX_CE && loss != SCS_LOSS_SOFTMAX_CE) ||
        (ggn == SCS_GGN_LINEAR_MULTI_LS && loss != SCS_LOSS_MULTI_LS) ||
        (multi_loss(loss) && ggn != SCS_GGN_NONE && ggn != SCS_GGN_LINEAR_SOFTMAX_CE && ggn != SCS_GGN_LINEAR_MULTI_LS))
      fail(c, SCS_ERR_ARG, "SCS_GGN_LINEAR_SOFTMAX_CE goes with SCS_LOSS_SOFTMAX_CE and SCS_GGN_LINEAR_MULTI_LS with "
                           "SCS_LOSS_MULTI_LS (got loss %d, ggn %d)", loss, ggn);
    if ((loss == SCS_LOSS_SAMPLEWISE) != (ggn == SCS_GGN_SAMPLEWISE) && !(loss == SCS_LOSS_SAMPLEWISE && ggn == SCS_GGN_NONE))
      fail(c, SCS_ERR_ARG, "SCS_LOSS_SAMPLEWISE takes SCS_GGN_NONE or SCS_GGN_SAMPLEWISE, and no other loss takes the latter");
    if (loss == SCS_LOSS_SAMPLEWISE) {
      if (!c->sw) fail(c, SCS_ERR_STATE, "no sample-wise loss functions: call scs_set_loss_samplewise first");
      if (scale != 1.0)
        fail(c, SCS_ERR_ARG, "a sample-wise loss takes scale = 1 (its values arrive scaled), got %g", scale);
      if (ggn == SCS_GGN_SAMPLEWISE && !c->sw_ggn)
        fail(c, SCS_ERR_ARG, "SCS_GGN_SAMPLEWISE needs the GGN pieces (scs_set_loss_samplewise with has_ggn)");
      if (c->has_data && c->generic)
        fail(c, SCS_ERR_ARG, "a sample-wise loss needs device data (A, y): this context is a ProblemGeneric");
    }
    if ((loss == SCS_LOSS_QUADRATIC || loss == SCS_LOSS_ROSENBROCK || loss == SCS_LOSS_CALLBACK) && sharded(c))
      fail(c, SCS_ERR_ARG, "quadratic / Rosenbrock / callback problems are not row-sharded");
    if (loss == SCS_LOSS_CALLBACK && (!c->has_data || !c->generic))
      fail(c, SCS_ERR_ARG, "a callback loss holds no device data: scs_set_data(N = 0, A = NULL, m) first");
    if (loss == SCS_LOSS_CALLBACK && ggn != SCS_GGN_NONE)
      fail(c, SCS_ERR_ARG, "a callback loss has no out_fn kind (its GGN pieces come from the callback)");
    if (loss == SCS_LOSS_QUADRATIC && ((c->has_data && !c->generic && !c->sparse && c->a32) || c->tset.v.a32))
      fail(c, SCS_ERR_ARG, "the quadratic loss needs an fp64-stored A: fp32 storage (scs_set_dense_f32 / "
                           "scs_set_data_f32) does not cover it");
    c->loss = loss;
    c->ggn = ggn;
    c->scale = scale;
    c->loss_set = true;
    ++c->data_gen;
    invalidate_caches(c);
  });
}

int scs_set_loss_samplewise(scs_ctx* c, scs_samplewise_fn* fn, void* user, int device_ptrs, int has_ggn) {
  if (is_group(c)) {
    c->err = "a sample-wise loss takes a single-device context (a group's devices run one host thread each)";
    return SCS_ERR_ARG;
  }
  return guarded(c, [&] {
    if (!fn && c->loss_set && c->loss == SCS_LOSS_SAMPLEWISE)
      fail(c, SCS_ERR_STATE, "the sample-wise loss is in use: select another loss before removing its functions");
    c->sw = fn;
    c->sw_user = user;
    c->sw_dev = device_ptrs != 0;
    c->sw_ggn = has_ggn != 0;
    invalidate_caches(c);
  });
}

int scs_set_loss_callback(scs_ctx* c, scs_loss_fn fn, void* user, int64_t ggn_rows) {
  return guarded(c, [&] {
    if (ggn_rows < 0) fail(c, SCS_ERR_ARG, "ggn_rows must be >= 0");
    c->cb = fn;
    c->cb_user = user;
    if (ggn_rows != c->cb_nout) {
      free_view(c, c->cbv);
      dfree_t(c, c->cbstage);
      c->cb_nout = ggn_rows;
    }
    invalidate_caches(c);
  });
}

static double* upload_bounds(scs_ctx* c, double* old, const double* v, int64_t nb, bool sanitize, bool lower) {
  dfree_t(c, old);
  std::vector<double> h(c->mpad, 0.0);
  for (int64_t i = 0; i < c->m; ++i) {
    double b = (nb == 1) ? v[0] : v[i];
    if (sanitize) {
      if (lower && b == -INFINITY) b = -1e32;  // L_INF_CACHE, prox-reg-utils.jl:6
      if (!lower && b == INFINITY) b = 1e32;   // U_INF_CACHE
    }
    h[i] = b;
  }
  double* d = dalloc<double>(c, c->mpad);
  h2d(c, d, h.data(), c->mpad);
  sync(c);
  return d;
}

int scs_set_reg(scs_ctx* c, int reg, const double* lam, int nlam, const double* lb, const double* ub, int64_t nbound,
                const int64_t* ind, int64_t ngroups) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_reg(s_, reg, lam, nlam, lb, ub, nbound, ind, ngroups); });
  return guarded(c, [&] {
    if (!c->has_data) fail(c, SCS_ERR_STATE, "set the data before the regularizer");
    if (reg < SCS_REG_L1 || reg > SCS_REG_GL) fail(c, SCS_ERR_REF, "reg_name not valid.");
    if (nlam < 1 || nlam > 2 || !lam) fail(c, SCS_ERR_ARG, "λ must have 1 or 2 entries");
    if (reg == SCS_REG_GL && nlam != 2)
      fail(c, SCS_ERR_REF, "Please provide a Tuple or Vector with exactly two entries for λ, e.g. [λ1, λ2]");
    c->reg = reg;
    c->nlam = nlam;
    c->lam = lam[0];  // step! uses λ = model.λ[1] when length(λ) > 1
    c->lam2 = nlam > 1 ? lam[1] : 0.0;
    if (reg == SCS_REG_INDBOX) {
      if (!lb || !ub || (nbound != 1 && nbound != c->m)) fail(c, SCS_ERR_ARG, "indbox needs C_set bounds (1 or m)");
      c->clb = upload_bounds(c, c->clb, lb, nbound, false, true);
      c->cub = upload_bounds(c, c->cub, ub, nbound, false, false);
    }
    if (reg == SCS_REG_GL) {
      if (!ind || ngroups < 1) fail(c, SCS_ERR_ARG, "gl needs the group index matrix");
      std::vector<int> hs(ngroups), he(ngroups);
      std::vector<double> hw(ngroups), wel(c->mpad, 0.0);
      // get_Cmat (prox-reg-utils.jl:121-142) needs the ranges to cover 1..n exactly once, in any
      // order (a gap leaves a zero column index, an overlap makes Cmat longer than x)
      std::vector<char> seen(c->m, 0);
      for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t s = ind[3 * g], e = ind[3 * g + 1], w = ind[3 * g + 2];
        if (s < 1 || e < s || e > c->m)
          fail(c, SCS_ERR_ARG, "group %lld = %lld:%lld is outside 1..%lld", (long long)g + 1, (long long)s,
               (long long)e, (long long)c->m);
        for (int64_t k = s - 1; k < e; ++k) {
          if (seen[k]) fail(c, SCS_ERR_ARG, "groups overlap at %lld: they must partition 1..m", (long long)k + 1);
          seen[k] = 1;
          wel[k] = (double)w;
        }
        hs[g] = (int)(s - 1);
        he[g] = (int)(e - 1);
        hw[g] = (double)w;
      }
      for (int64_t k = 0; k < c->m; ++k)
        if (!seen[k]) fail(c, SCS_ERR_ARG, "groups must partition 1..m (%lld is in no group)", (long long)k + 1);
      dfree_t(c, c->gmap);
      dfree_t(c, c->gstart);
      dfree_t(c, c->gend);
      dfree_t(c, c->gw);
      dfree_t(c, c->wel);
      c->gstart = dalloc<int>(c, ngroups);
      c->gend = dalloc<int>(c, ngroups);
      c->gw = dalloc<double>(c, ngroups);
      c->wel = dalloc<double>(c, c->mpad);
      HCK(hipMemcpyAsync(c->gstart, hs.data(), sizeof(int) * ngroups, hipMemcpyHostToDevice, c->st));
      HCK(hipMemcpyAsync(c->gend, he.data(), sizeof(int) * ngroups, hipMemcpyHostToDevice, c->st));
      h2d(c, c->gw, hw.data(), ngroups);
      h2d(c, c->wel, wel.data(), c->mpad);
      c->ngroups = (int)ngroups;
      sync(c);
    }
    c->reg_set = true;
  });
}

int scs_set_compute_f32(scs_ctx* c, int on) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_compute_f32(s_, on); });
  return guarded(c, [&] {
    if (on) refuse_multi(c, "scs_set_compute_f32 (the fp32-arithmetic products have one right-hand side)");
    sync(c);
    c->f32c = on ? 1 : 0;
    invalidate_caches(c);
  });
}

int scs_set_solver(scs_ctx* c, int kind) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_solver(s_, kind); });
  return guarded(c, [&] {
    if (kind != SCS_SOLVER_DEFAULT && kind != SCS_SOLVER_REFERENCE) fail(c, SCS_ERR_ARG, "scs_set_solver: kind %d", kind);
    c->solver = kind;
  });
}

int scs_set_gram_cache(scs_ctx* c, int on) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_gram_cache(s_, on); });
  return guarded(c, [&] {
    c->gram_cache = on ? 1 : 0;
    ++c->data_gen;
    if (!on) dfree_t(c, c->Gk);
  });
}

int scs_set_group_map(scs_ctx* c, const int64_t* G, int64_t ntotal) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_group_map(s_, G, ntotal); });
  return guarded(c, [&] {
    if (!c->reg_set || c->reg != SCS_REG_GL) fail(c, SCS_ERR_STATE, "scs_set_group_map needs reg gl set first");
    if (!G || ntotal != c->m)
      fail(c, SCS_ERR_ARG, "G must select every variable once (length %lld, m = %lld)", (long long)ntotal,
           (long long)c->m);
    std::vector<int> h(ntotal);
    std::vector<char> seen(c->m, 0);
    bool ident = true;
    for (int64_t k = 0; k < ntotal; ++k) {
      if (G[k] < 1 || G[k] > c->m || seen[G[k] - 1]) fail(c, SCS_ERR_ARG, "G must be a permutation of 1..m");
      seen[G[k] - 1] = 1;
      h[k] = (int)(G[k] - 1);
      ident = ident && (G[k] == k + 1);
    }
    dfree_t(c, c->gmap);
    if (ident) return;
    c->gmap = dalloc<int>(c, ntotal);
    HCK(hipMemcpyAsync(c->gmap, h.data(), sizeof(int) * ntotal, hipMemcpyHostToDevice, c->st));
    sync(c);
  });
}

int scs_set_smoother(scs_ctx* c, int kind, double mu, double Mh, double nu, const double* lb, const double* ub,
                     int64_t nbound) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_smoother(s_, kind, mu, Mh, nu, lb, ub, nbound); });
  return guarded(c, [&] {
    if (!c->has_data) fail(c, SCS_ERR_STATE, "set the data before the smoother");
    if (kind < SCS_SMOOTH_PHUBER_L1L2 || kind > SCS_SMOOTH_OSBA_GL) fail(c, SCS_ERR_ARG, "unknown smoother %d", kind);
    if (kind == SCS_SMOOTH_PHUBER_INDBOX || kind == SCS_SMOOTH_EXP_INDBOX || kind == SCS_SMOOTH_LOGEXP_INDBOX) {
      if (!lb || !ub || (nbound != 1 && nbound != c->m))
        fail(c, SCS_ERR_REF, "Lengths of the bounds do not match that of the variable.");
      c->slb = upload_bounds(c, c->slb, lb, nbound, true, true);
      c->sub = upload_bounds(c, c->sub, ub, nbound, true, false);
    }
    if ((kind == SCS_SMOOTH_PHUBER_GL || kind == SCS_SMOOTH_OSBA_GL) && !c->wel)
      fail(c, SCS_ERR_STATE, "%s needs the gl groups (scs_set_reg)",
           kind == SCS_SMOOTH_PHUBER_GL ? "PHuberSmootherGL" : "OsBaSmootherGL");
    c->smooth = kind;
    c->mu = mu;
    c->Mh = Mh;
    c->nu = nu;
    c->smooth_set = true;
    invalidate_caches(c);
  });
}

int scs_set_L(scs_ctx* c, int has_L, double L) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_L(s_, has_L, L); });
  return guarded(c, [&] {
    c->has_L = has_L != 0;
    c->L = L;
  });
}

int scs_method_init(scs_ctx* c, int method, int ss_type, int use_prox, int mem) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_method_init(s_, method, ss_type, use_prox, mem); });
  return guarded(c, [&] {
    if (!c->has_data) fail(c, SCS_ERR_STATE, "set the data before the method");
    if (method < SCS_PROX_NSCORE || method > SCS_PROX_LQNSCORE) fail(c, SCS_ERR_ARG, "unknown method %d", method);
    if (method == SCS_PROX_GGNSCORE && c->loss == SCS_LOSS_CALLBACK && c->cb_nout <= 0)
      fail(c, SCS_ERR_ARG, "ProxGGNSCORE on a callback loss needs jac_yx / grad_fy / hess_fy (ggn_rows > 0)");
    if (method == SCS_PROX_GGNSCORE && c->loss != SCS_LOSS_CALLBACK && (c->generic || c->loss == SCS_LOSS_QUADRATIC))
      fail(c, SCS_ERR_ARG, "ProxGGNSCORE needs a data problem with an out_fn (GGN kind)");
    refuse_multi_sample_space(c, method);
    c->method = method;
    c->ss_type = ss_type;
    c->use_prox = use_prox;
    c->mem = mem;
    if (method == SCS_PROX_LQNSCORE) {
      if (mem < 1) fail(c, SCS_ERR_ARG, "L-BFGS memory must be >= 1");
      dfree_t(c, c->S);
      dfree_t(c, c->Yv);
      dfree_t(c, c->d_order);
      dfree_t(c, c->ab);
      dfree_t(c, c->tlwork);
      c->tlwork = dalloc<double>(c, (size_t)(mem + 5) * TWO_LOOP_MAX_WG);
      c->S = dalloc<double>(c, (size_t)(mem + 1) * c->mpad);
      c->Yv = dalloc<double>(c, (size_t)(mem + 1) * c->mpad);
      c->d_order = dalloc<int>(c, mem + 3);   // order[0..mem] | k | spare (the device ring)
      if (c->hring) (void)hipHostFree(c->hring);
      c->hring = nullptr;
      HCK(hipHostMalloc((void**)&c->hring, sizeof(int) * (mem + 3), hipHostMallocDefault));
      c->ab = dalloc<double>(c, 2 * (mem + 1));
      sync(c);
    }
    // init! (prox-L-BFGS-SCORE.jl:31-36)
    c->ring.clear();
    c->spare = 0;
    c->H0 = 1.0;
    c->lbfgs_pending = false;
    c->method_set = true;
    invalidate_caches(c);
    // scs_set_sparse_batches: a pool view is sparse (ProxLQNSCORE) or dense (the Gram methods); views of
    // the other kind go, and a selected batch gets its view of the right kind
    // (scs_set_sparse_sample: ProxGGNSCORE's sparse views also hold what the sample space reads, so
    // ProxLQNSCORE's views do not serve it; its batches of the feature branch stay dense)
    if (c->sparse_batches && c->sparse) {
      const int kind = batch_view_kind(c, method);
      const bool drop_dense = !c->bpool.empty() && (kind == 1 || (kind == 2 && c->vkind != 2));
      const bool drop_sparse = !c->spool.empty() && c->spool_kind != kind;
      c->vkind = kind;
      if (drop_dense || drop_sparse) {
        sync(c);
        if (drop_dense) free_dense_views(c);
        if (drop_sparse) free_sparse_views(c);
        if (c->bsel >= 0) select_batch(c, c->bsel);
      }
    }
  });
}

int scs_eval_f(scs_ctx* c, const double* x, double* fval) {
  if (is_group(c)) return group_eval(c, x, fval, 1, scs_eval_f);
  return guarded(c, [&] {
    if (!c->has_data) fail(c, SCS_ERR_STATE, "no data: call scs_set_data / scs_gen_data first");
    if (!c->loss_set) fail(c, SCS_ERR_STATE, "no loss: call scs_set_loss first");
    HCK(hipSetDevice(c->dev));
    h2d(c, c->xn, x, c->m);
    *fval = eval_f_dev(c, x, c->xn);
  });
}

int scs_eval_grad(scs_ctx* c, const double* x, double* g) {
  if (is_group(c)) return group_eval(c, x, g, c->grpm, scs_eval_grad);
  return guarded(c, [&] {
    if (!c->has_data) fail(c, SCS_ERR_STATE, "no data: call scs_set_data / scs_gen_data first");
    if (!c->loss_set) fail(c, SCS_ERR_STATE, "no loss: call scs_set_loss first");
    HCK(hipSetDevice(c->dev));
    h2d(c, c->xn, x, c->m);
    grad_f_dev(c, x, c->xn, c->gqn);
    d2h(c, g, c->gqn, c->m);
    sync(c);
  });
}

int scs_eval_reg(scs_ctx* c, const double* x, double* gval) {
  if (is_group(c)) return group_eval(c, x, gval, 1, scs_eval_reg);
  return guarded(c, [&] {
    require_ready(c, false);
    HCK(hipSetDevice(c->dev));
    h2d(c, c->xn, x, c->m);
    *gval = eval_reg_dev(c, c->xn);
  });
}

int scs_set_batches(scs_ctx* c, const int64_t* rows, const int64_t* offsets, int64_t nbatch) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_set_batches(s_, rows, offsets, nbatch); });
  return guarded(c, [&] {
    HCK(hipSetDevice(c->dev));
    sync(c);
    clear_batches(c);
    invalidate_caches(c);
    if (nbatch == 0) return;
    if (multi(c) && !c->multi_batches)
      fail(c, SCS_ERR_ARG, "scs_set_batches: minibatches (batch_size / slice_samples) are not supported with "
                           "scs_set_outputs (nout = %d) unless multi_batches / scs_set_multi_batches is on", c->nout);
    if (!c->has_data) fail(c, SCS_ERR_STATE, "no data: call scs_set_data / scs_gen_data first");
    if (multi(c) && c->sparse && !c->multi_sparse_batches)
      fail(c, SCS_ERR_ARG, "scs_set_batches: minibatches with scs_set_outputs (nout = %d) need a dense A (a sparse A, "
                           "scs_set_sparse_outputs included, is not supported with multi_batches / "
                           "scs_set_multi_batches) unless multi_sparse_batches / scs_set_multi_sparse_batches is on",
           c->nout);
    if (multi(c) && !c->sparse) c->mb_gather = multi_gather_arm(c->a32);
    if (multi(c) && c->sparse) c->msb_narrow = multi_narrow_form(c->nout, c->sp_f32);
    if (c->generic) fail(c, SCS_ERR_ARG, "a ProblemGeneric has no samples to batch");
    if (nbatch < 0 || !rows || !offsets || offsets[0] != 0) fail(c, SCS_ERR_ARG, "scs_set_batches: bad batch list");
    for (int64_t b = 0; b < nbatch; ++b)
      if (offsets[b + 1] <= offsets[b]) fail(c, SCS_ERR_ARG, "scs_set_batches: batch %lld is empty", (long long)b);
    const int64_t tot = offsets[nbatch];
    // rows are global indices (row0 = 0, Nglob = N on one rank): keep this rank's rows of each batch
    for (int64_t i = 0; i < tot; ++i)
      if (rows[i] < 0 || rows[i] >= c->Nglob)
        fail(c, SCS_ERR_ARG, "scs_set_batches: row %lld out of range", (long long)rows[i]);
    std::vector<int64_t> loc;
    c->boff.assign(1, 0);
    for (int64_t b = 0; b < nbatch; ++b) {
      for (int64_t i = offsets[b]; i < offsets[b + 1]; ++i)
        if (rows[i] >= c->row0 && rows[i] < c->row0 + c->N) {
          loc.push_back(rows[i] - c->row0);
          c->bpos.push_back(i - offsets[b]);
        }
      c->boff.push_back((int64_t)loc.size());
      c->bglob.push_back(offsets[b + 1] - offsets[b]);
    }
    c->brows = dalloc<int64_t>(c, std::max<size_t>(loc.size(), 1));
    if (!loc.empty())
      HCK(hipMemcpyAsync(c->brows, loc.data(), sizeof(int64_t) * loc.size(), hipMemcpyHostToDevice, c->st));
    sync(c);
    // the kept sparse views' budget: the bytes the sparse data takes now, or SCS_SPARSE_BATCH_CACHE_MB
    c->bplan.reset(scs::batch_budget_bytes(std::getenv("SCS_SPARSE_BATCH_CACHE_MB"),
                                           c->sparse ? sparse_data_bytes(c) : 0));
    // the exchange payload of the new list's sample-space batches (reduce_buffer_doubles)
    if (c->own_red && c->red && reduce_buffer_doubles(c) > c->red_cap) {
      dfree_t(c, c->red);
      c->red_cap = 0;
      c->own_red = false;
      ensure_red(c);
    }
  });
}

int scs_select_batch(scs_ctx* c, int64_t b) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_select_batch(s_, b); });
  return guarded(c, [&] {
    const int64_t nb = c->boff.empty() ? 0 : (int64_t)c->boff.size() - 1;
    if (b < -1 || b >= nb) fail(c, SCS_ERR_ARG, "scs_select_batch: batch %lld of %lld", (long long)b, (long long)nb);
    HCK(hipSetDevice(c->dev));
    select_batch(c, b);
    sync(c);
  });
}

static void step_call(scs_ctx* c, const double* x, const double* x_prev, int64_t iter, const double* grad_fx,
                      double* x_new, double* dx, double* pri) {
  require_ready(c, true);
  HCK(hipSetDevice(c->dev));
  hipEvent_t e0;
  tbegin(c, T_STEP, &e0);
  BatchScope bs(c);
  h2d(c, c->x, x, c->m);
  h2d(c, c->xp, x_prev ? x_prev : x, c->m);
  std::vector<double> xnew_h(c->m);
  {
    // ∇fx lives in its own buffer for the call (gtmp2 is line-search scratch)
    double* gbuf = nullptr;
    // ProxGGNSCORE takes ∇fx and never reads it (prox-GGN-SCORE.jl:34-135: its grad_f -- the line
    // search's ∇q, :58-63,83-84 -- is the model's gradient): only NSCORE / LQN install it
    if (grad_fx && c->method != SCS_PROX_GGNSCORE) {
      gbuf = dalloc<double>(c, c->mpad);
      h2d(c, gbuf, grad_fx, c->m);
      invalidate_caches(c);
      c->gfix = gbuf;
    }
    struct Release {
      scs_ctx* c;
      double* g;
      ~Release() {
        if (!g) return;
        c->gfix = nullptr;
        invalidate_caches(c);
        (void)hipStreamSynchronize(c->st);
        dfree_t(c, g);
      }
    } rel{c, gbuf};
    if (c->method == SCS_PROX_LQNSCORE)
      step_lqn(c, x, x_prev ? x_prev : x, iter, xnew_h.data(), dx, pri);
    else
      step_newton(c, x, iter, xnew_h.data(), dx, pri);
  }
  std::memcpy(x_new, xnew_h.data(), sizeof(double) * c->m);
  tend(c, T_STEP, e0);
  if (c->timing) tresolve(c);
}

int scs_step(scs_ctx* c, const double* x, const double* x_prev, int64_t iter, double* x_new, double* dx,
             double* pri) {
  if (is_group(c)) return group_step(c, x, x_prev, iter, nullptr, x_new, dx, pri);
  return guarded(c, [&] { step_call(c, x, x_prev, iter, nullptr, x_new, dx, pri); });
}

int scs_step_grad(scs_ctx* c, const double* x, const double* x_prev, int64_t iter, const double* grad_fx,
                  double* x_new, double* dx, double* pri) {
  if (is_group(c)) return group_step(c, x, x_prev, iter, grad_fx, x_new, dx, pri);
  return guarded(c, [&] { step_call(c, x, x_prev, iter, grad_fx, x_new, dx, pri); });
}

// optim_loop! (iterate.jl:100-267), full-batch, in C++ around the same device calls the
// per-call entry points make (f(x) + get_reg(x) + step! per epoch), so a caller pays one
// ABI crossing per solve instead of three per epoch.  Histories follow iterate.jl exactly:
// one push per epoch (the pre-step values), the duplicated entry at max_epoch
// (:219-231) or the post-step entry on termination (:235-247); pri_res_norm[0] is
// `nothing` (NaN here).  Termination uses the pre-step f_rel_error (:234, :257).
// scs_iterate: the r03 six-field history (obj .. times) -- fvaltest is never read or written
int scs_iterate(scs_ctx* c, const double* x0, const double* x_star, int64_t max_epoch, double x_tol, double f_tol,
                int rel_kind, double* x_out, const scs_history* h, int64_t* n_hist, int64_t* epochs_out) {
  // r05 made this entry the six-field (r03) layout: it never writes fvaltest.  A context that holds test
  // data expects Solution.fvaltest, which only scs_iterate_ex returns -- refused rather than dropped
  // silently (r04 C callers: call scs_iterate_ex with sizeof(scs_history))
  int on = 0;
  if (c && scs_has_test(c, &on) == SCS_OK && on) {
    c->err = "scs_iterate has no fvaltest (six-field history) and this context holds test data: call scs_iterate_ex "
             "with sizeof(scs_history)";
    return SCS_ERR_STATE;
  }
  return scs_iterate_ex(c, x0, x_star, max_epoch, x_tol, f_tol, rel_kind, x_out, h, offsetof(scs_history, fvaltest),
                        n_hist, epochs_out);
}

int scs_iterate_ex(scs_ctx* c, const double* x0, const double* x_star, int64_t max_epoch, double x_tol, double f_tol,
                   int rel_kind, double* x_out, const scs_history* hist, size_t hist_size, int64_t* n_hist,
                   int64_t* epochs_out) {
  // the caller's struct as far as it reaches (a shorter, older layout leaves the later fields NULL)
  scs_history hcopy{};
  if (hist) std::memcpy(&hcopy, hist, std::min(hist_size, sizeof(scs_history)));
  const scs_history* h = hist ? &hcopy : nullptr;
  if (is_group(c)) return group_iterate(c, x0, x_star, max_epoch, x_tol, f_tol, rel_kind, x_out, h, n_hist, epochs_out);
  return guarded(c, [&] {
    require_ready(c, true);
    if (!x0 || !x_star || !x_out || !h || !n_hist || !epochs_out) fail(c, SCS_ERR_ARG, "scs_iterate: null argument");
    if (hist_size < offsetof(scs_history, fvaltest))
      fail(c, SCS_ERR_ARG, "scs_iterate_ex: hist_size %zu < the six history arrays", hist_size);
    if (max_epoch < 1) fail(c, SCS_ERR_ARG, "scs_iterate: max_epoch must be >= 1");
    HCK(hipSetDevice(c->dev));
    const int64_t m = c->m;
    // Σ (a − b)² (b may be null) in a fixed order: eight interleaved partial sums (vectorized;
    // the one-accumulator loop was ~90 us per call at m = 65536, three calls per epoch, on the
    // C5 step's critical path), then a fixed tree and the tail.  Julia's norm is BLAS nrm2, a
    // different order again; termination compares at x_tol, not ulps.
    auto sumsq = [&](const double* a, const double* b) {
      double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      int64_t i = 0;
      if (b) {
        for (; i + 8 <= m; i += 8)
          for (int l = 0; l < 8; ++l) {
            const double d = a[i + l] - b[i + l];
            acc[l] += d * d;
          }
      } else {
        for (; i + 8 <= m; i += 8)
          for (int l = 0; l < 8; ++l) acc[l] += a[i + l] * a[i + l];
      }
      double t = 0.0;
      for (; i < m; ++i) {
        const double d = b ? a[i] - b[i] : a[i];
        t += d * d;
      }
      return (((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))) + t;
    };
    auto nrm = [&](const double* a, const double* b) { return std::sqrt(sumsq(a, b)); };   // ‖a − b‖
    auto jmax = [](double a, double b) {   // Julia max: NaN propagates, -0.0 < +0.0
      if (std::isnan(a)) return a;
      if (std::isnan(b)) return b;
      return (b < a || (std::signbit(b) && !std::signbit(a))) ? a : b;
    };
    // f(x) + get_reg(x) with one upload of x (c->xn holds it for both)
    // the tagged host vector the device buffers c->x / c->xn hold (0: unknown), so a vector
    // already on the device is not uploaded again (x = the last step's x_new = c->xn)
    uint64_t dev_x = 0, dev_xn = 0;
    auto fobj_of = [&](const double* xx, double* fv) {
      const uint64_t t = xtag_of(c, xx);
      if (!(t && t == dev_xn)) {
        h2d(c, c->xn, xx, m);
        dev_xn = t;
      }
      *fv = eval_f_dev(c, xx, c->xn);
      return *fv + eval_reg_dev(c, c->xn);
    };
    // ftest(x) of a host vector (uploaded to c->xn unless it is already there, as fobj_of)
    auto ftest_of = [&](const double* xx) -> double {
      if (!c->tset.on) return std::numeric_limits<double>::quiet_NaN();
      const uint64_t t = xtag_of(c, xx);
      if (!(t && t == dev_xn)) {
        h2d(c, c->xn, xx, m);
        dev_xn = t;
      }
      return eval_ftest_dev(c, xx, c->xn);
    };
    const double nstar = nrm(x_star, nullptr);
    auto rel_of = [&](const double* xx) {
      if (rel_kind == 1) return sumsq(x_star, xx) / (double)m;   // mean_square_error (utils.jl:3-5), the "gl" rel_error
      return jmax(nrm(xx, x_star) / jmax(nstar, 1.0), x_tol);
    };
    const auto t0 = std::chrono::steady_clock::now();
    auto now = [&] {   // Dates.now() differences: millisecond resolution
      const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      return std::floor(sec * 1000.0) / 1000.0;
    };
    double fstar = 0.0;
    const double obj_star = fobj_of(x_star, &fstar);
    auto frel_of = [&](double ob) { return jmax(std::fabs(ob - obj_star) / std::fabs(obj_star), f_tol); };
    int64_t nh = 0;
    // show_stat! + update_stat! (utils.jl:50-57,106-113): with held-out data every push carries
    // ftest of the pushed point too (the `fvaltests` vector, iterate.jl:169-175), so the test
    // history has one entry per obj entry
    const bool tst = c->tset.on;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto push = [&](double ob, double fv, double pr, double rl, double fr, double dt, double ft) {
      if (c->tset.xor_case)   // iterate.jl:170-171 then :201: ftest is unassigned at the first show_stat!
        fail(c, SCS_ERR_REF, "UndefVarError: `ftest` not defined (only one of Atest / ytest was given: "
                             "iterate.jl:170-171 leave ftest unassigned, show_stat! at :201 reads it)");
      h->obj[nh] = ob;
      h->fval[nh] = fv;
      h->pri_res_norm[nh] = pr;
      h->rel[nh] = rl;
      h->objrel[nh] = fr;
      if (h->times) h->times[nh] = dt;
      if (tst && h->fvaltest) h->fvaltest[nh] = ft;
      ++nh;
    };
    // init!(method, x): reset the method state (prox-L-BFGS-SCORE.jl:31-36)
    c->ring.clear();
    c->spare = 0;
    c->H0 = 1.0;
    c->lbfgs_pending = false;
    invalidate_caches(c);
    // x, x_prev, x_new in pinned host memory: their per-epoch uploads / the x_new download are
    // DMA transfers instead of staged pageable copies (the arrays are only touched after syncs)
    struct Pinned {
      double* p = nullptr;
      ~Pinned() {
        if (p) (void)hipHostFree(p);
      }
    } pin;
    HCK(hipHostMalloc((void**)&pin.p, sizeof(double) * 3 * std::max<int64_t>(m, 1), hipHostMallocDefault));
    double* x = pin.p;
    double* x_prev = pin.p + m;
    double* x_new = pin.p + 2 * m;
    std::memcpy(x, x0, sizeof(double) * m);
    std::memcpy(x_prev, x0, sizeof(double) * m);
    // version tags of the three buffers for the f / ∇q caches (unregistered on exit)
    struct Untag {
      scs_ctx* c;
      ~Untag() {
        for (auto& t : c->xtags) t = scs_ctx::XTag{};
      }
    } untag{c};
    auto tag_slot = [&](const double* p) -> scs_ctx::XTag& {
      for (auto& t : c->xtags)
        if (t.p == p) return t;
      fail(c, SCS_ERR_STATE, "scs_iterate: untracked buffer");
      return c->xtags[0];
    };
    c->xtags[0] = {x, c->xtag_next};
    c->xtags[1] = {x_prev, c->xtag_next++};   // same content as x
    c->xtags[2] = {x_new, c->xtag_next++};
    double pri = std::numeric_limits<double>::quiet_NaN();
    int64_t epochs = 0;
    // the collected batches (iterate.jl:146): the registered list, else the one full batch
    const int64_t nb = c->boff.empty() ? 0 : (int64_t)c->boff.size() - 1;
    const int64_t iend = std::max<int64_t>(nb, 1);
    struct Unselect {
      scs_ctx* c;
      ~Unselect() { unselect_view(c); }
    } unselect{c};
    double last_nx = 0.0, last_ndx = 0.0;
    // Device-resident loop (the full batch of a data loss): x, x_prev, x_new never leave the
    // device; get_reg(x), f(x), rel_error and the two norms of the termination test are reduced
    // on the device and read back with pri_res_norm (and L-BFGS's δhᵀγh) in ONE copy + sync at the
    // end of each epoch -- the GPU only idles for that hand-off.  Same kernels, same order as the
    // per-call path, so the histories equal the host loop's (the norms differ in summation order
    // only; test_device_loop_matches_host_loop).
    // (a Rosenbrock ProblemGeneric runs here too: its f / ∇f / ∇²f are device kernels; the
    // quadratic loss and the host callbacks keep the per-call path)
    const bool dev_ok = nb == 0 && c->loss != SCS_LOSS_QUADRATIC && c->loss != SCS_LOSS_CALLBACK &&
                        (!c->generic || c->loss == SCS_LOSS_ROSENBROCK);
    if (dev_ok) {
      struct DevLoop {
        scs_ctx* c;
        explicit DevLoop(scs_ctx* cc) : c(cc) { c->dev_loop = true; }
        ~DevLoop() { c->dev_loop = false; }
      } devloop(c);
      h2d(c, c->xstar, x_star, m);
      h2d(c, c->x, x0, m);
      HCK(hipMemcpyAsync(c->xp, c->x, sizeof(double) * m, hipMemcpyDeviceToDevice, c->st));
      double* hs = c->hscal;
      auto rel_from = [&](double ss) {
        if (rel_kind == 1) return ss / (double)m;
        return jmax(std::sqrt(ss) / jmax(nstar, 1.0), x_tol);
      };
      // ProxLQNSCORE, fused epoch (lqn_tail / lqn_post, vec.hip): 7 launches per epoch around the two
      // products instead of ~22; every quantity the history and the termination test read for the
      // NEXT x is produced by this epoch's post pass, so the hand-off at the epoch end is the only
      // one.  Same per-element arithmetic and partial-sum order as the unfused step (bit-identical
      // x, obj, fval, pri_res_norm; SCS_LQN_FUSED=0 selects the unfused epoch).
      const char* fz = std::getenv("SCS_LQN_FUSED");
      const bool fused = c->method == SCS_PROX_LQNSCORE && c->ss_type == 1 && m >= 16384 && !sharded(c) &&
                         c->smooth != SCS_SMOOTH_PHUBER_GL && c->smooth != SCS_SMOOTH_OSBA_GL &&
                         !(c->use_prox && c->reg == SCS_REG_GL) && c->reg != SCS_REG_GL && !(fz && fz[0] == '0') &&
                         c->loss != SCS_LOSS_SAMPLEWISE &&   // its epoch is pipelined past the caller's functions
                         !multi(c);   // the fused epoch's post pass reads single-vector Aᵀv partials
      if (fused) {
        const double Mg = get_Mg(c, c->Mh, c->nu, c->mu, m);
        const double step = c->has_L ? jl_min_h(1 / c->L, 1.0) : 0.5;
        // state at x0: ∇q(x0) -> gq, then smoother(x0) -> gr, Hr, hinv and η's partials, f / get_reg / norms
        grad_q_dev(c, x, c->x, c->gq);
        HCK(launch_smoother(c->smooth, c->x, m, c->mu, c->slb, c->sub, c->wel, c->gr, c->Hr, c->st));
        HCK(launch_lqn_eta(c->gr, c->Hr, m, c->lam, c->hinv, c->lqR, c->st));
        HCK(launch_reg_value(prox_args(c), c->x, m, c->scal + RX_SLOT, c->scal + 64 + 2 * 256, c->st));
        HCK(launch_norms3(c->x, c->xstar, nullptr, m, c->scal + NRM_SLOT, c->scal + 64 + 3 * 256, c->st));
        forward(c, x, c->x, 0, false);   // cached: the z of x0 from ∇q(x0)
        if (tst) ftest_enqueue(c, c->x);
        d2h(c, hs, c->scal, LOOP_SLOTS);
        sync(c);
        double fcur = loss_scale_value(c, hs[ZF_SLOT]), regcur = hs[RX_SLOT];
        double ftcur = tst ? loss_scale_value(c, hs[TF_SLOT]) : nan;
        double relcur = rel_from(hs[NRM_SLOT]), nxcur = std::sqrt(hs[NRM_SLOT + 1]);
        // Pipelined by one epoch: epoch e+1 is enqueued before the host reads epoch e's scalars, so
        // the GPU never idles for the hand-off.  What the next epoch needs from this one stays on
        // the device: the L-BFGS ring ([order | k | spare] in d_order, H0 in scal[H0_SLOT]) is
        // advanced by lqn_post's last workgroup, and the two-loop launches for an upper bound of k
        // (the ring grows by at most one per epoch in flight; surplus launches return at once).
        // The host keeps the mirror (lbfgs_accept on the same δhᵀγh, γhᵀγh) for the history and
        // the state after the call.  An epoch enqueued past the stopping one writes only x_prev's
        // buffer, the spare pair slot and scratch; its buffer rotation is undone.
        const int mem = c->mem;
        for (int i = 0; i < mem + 3; ++i) c->hring[i] = 0;   // init!: empty ring, spare slot 0
        HCK(hipMemcpyAsync(c->d_order, c->hring, sizeof(int) * (mem + 3), hipMemcpyHostToDevice, c->st));
        HCK(launch_fill(c->scal + H0_SLOT, 1, 1.0, c->st));
        for (auto& ev : c->loop_ev)
          if (!ev) HCK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        struct Rot {
          double *x, *xp, *xn, *gq, *gqn;
        };
        auto rot_get = [&] { return Rot{c->x, c->xp, c->xn, c->gq, c->gqn}; };
        // the epoch's scalars: written by lqn_post's final kernel straight into the pinned buffer
        // (SCS_LOOP_HOSTMAP=0: a device-to-host copy after it)
        const char* hm_env = std::getenv("SCS_LOOP_HOSTMAP");
        const bool hostmap = !(hm_env && hm_env[0] == '0');
        int64_t enq = 0, done = 0;
        Rot before_last{};   // the rotation state before the latest enqueue
        // k = 0 is speculated while the host's ring is empty (no two-loop launches: the tail takes
        // d = -∇q); when the epoch in flight turns out to have accepted the first pair, the epoch
        // enqueued behind it is discarded and re-run (once per call: the ring never empties).
        bool spec_k0 = false;   // the latest enqueue assumed k = 0
        auto enqueue = [&](int64_t e) {
          before_last = rot_get();
          const bool timed = c->timing && (e % c->timing_every == 0);
          const bool tsave = c->timing;
          c->timing = timed;   // timing events cost a dispatch gap each: sample the epochs
          const int kmax = c->ring.empty() ? 0 : std::min<int>(mem, (int)c->ring.size() + (int)(enq - done));
          spec_k0 = kmax == 0;
          hipEvent_t e0;
          tbegin(c, T_STEP, &e0);
          if (kmax > 0)
            HCK(launch_two_loop(c->S, c->Yv, c->mpad, c->d_order, kmax, 1.0, c->gq, m, c->q, c->d, c->ab, c->tlwork,
                                mem, c->d_order + mem + 1, c->scal + H0_SLOT, c->st, c->f32c));
          HCK(launch_lqn_tail(c->x, kmax > 0 ? c->d : c->gq, kmax > 0 ? 0 : 1, m, Mg, step, prox_args(c), c->hinv,
                              c->xn, c->dxv, c->q, c->lqR, c->scal, c->st));
          if (tst) ftest_enqueue(c, c->xn);   // -> scal[TF_SLOT], carried to the host by lqn_post_final
          // z = A x_new, r = ∂f/∂z, f(x_new) -> scal[ZF_SLOT] (forward()'s passes, no host copies)
          hipEvent_t e1;
          tbegin(c, T_GEMV, &e1);
          const int ns = matvec_n(c, c->xn, c->nsplit);
          tend(c, T_GEMV, e1);
          HCK(launch_epilogue(c->loss, c->ggn, EPI_GRAD | EPI_Z | EPI_VAL, c->zpart, ns, c->Npad, c->y, c->N, c->Npad,
                              c->scale, c->z, c->gN, c->hN, c->wN, c->vN, c->valpart, c->st));   // Σ: lqn_post
          hipEvent_t e2;
          tbegin(c, T_GEMV, &e2);
          const int np = matvec_t_part(c, c->gN);       // Aᵀ r partials
          tend(c, T_GEMV, e2);
          HCK(launch_lqn_post(c->tpart, np, c->mpad, m, c->lam, c->smooth, c->mu, c->slb, c->sub, prox_args(c),
                              c->xstar, c->x, c->xn, c->gq, c->q, c->gqn, c->S, c->Yv, c->mpad, c->d_order, mem, 0,
                              c->gr, c->Hr, c->hinv, c->lqR, c->valpart, c->nval, c->scal, ZF_SLOT, RX_SLOT, NRM_SLOT,
                              H0_SLOT, c->hloop_dev + (e & 1) * LOOP_SLOTS, hostmap ? LOOP_SLOTS : 0, c->st));
          tend(c, T_STEP, e0);
          if (!hostmap) d2h(c, c->hloop + (e & 1) * LOOP_SLOTS, c->scal, LOOP_SLOTS);
          HCK(hipEventRecord(c->loop_ev[e & 1], c->st));
          double* t = c->xp;   // x_prev <- x, x <- x_new
          c->xp = c->x;
          c->x = c->xn;
          c->xn = t;
          std::swap(c->gq, c->gqn);   // ∇q(x) of the next epoch
          ++enq;
          c->timing = tsave;
        };
        auto restore_last = [&] {   // undo the rotation of the latest enqueue
          c->x = before_last.x;
          c->xp = before_last.xp;
          c->xn = before_last.xn;
          c->gq = before_last.gq;
          c->gqn = before_last.gqn;
        };
        enqueue(1);
        for (int64_t epoch = 1; epoch <= max_epoch; ++epoch) {
          const double dt = now();
          const double obj = fcur + regcur;
          const double frel = frel_of(obj);
          push(obj, fcur, pri, relcur, frel, dt, ftcur);
          if (epoch == max_epoch) push(obj, fcur, pri, relcur, frel, now(), ftcur);   // iterate.jl:219-231
          if (epoch < max_epoch) enqueue(epoch + 1);
          HCK(hipEventSynchronize(c->loop_ev[epoch & 1]));
          const double* he = c->hloop + (epoch & 1) * LOOP_SLOTS;
          ++done;
          const bool was_empty = c->ring.empty();
          lbfgs_accept(c, c->spare, he[16], he[17]);   // the device took the same decision
          if (was_empty && !c->ring.empty() && enq > done && spec_k0) {
            // epoch + 1 ran with d = -∇q but the memory now holds a pair: discard it.  Restore the
            // rotation, the ring (host mirror) and H0, and the smoother / η state at x_{epoch+1}
            // that its post pass overwrote (the same kernels as the setup), then enqueue it again.
            sync(c);
            restore_last();
            enq = done;
            const int k = (int)c->ring.size();
            for (int i = 0; i < mem + 3; ++i) c->hring[i] = 0;
            for (int i = 0; i < k; ++i) c->hring[i] = c->ring[i];
            c->hring[mem + 1] = k;
            c->hring[mem + 2] = c->spare;
            HCK(hipMemcpyAsync(c->d_order, c->hring, sizeof(int) * (mem + 3), hipMemcpyHostToDevice, c->st));
            HCK(launch_fill(c->scal + H0_SLOT, 1, c->H0, c->st));
            HCK(launch_smoother(c->smooth, c->x, m, c->mu, c->slb, c->sub, c->wel, c->gr, c->Hr, c->st));
            HCK(launch_lqn_eta(c->gr, c->Hr, m, c->lam, c->hinv, c->lqR, c->st));
            enqueue(epoch + 1);
          }
          pri = he[0];
          const double ndx = std::sqrt(he[NRM_SLOT + 2]);
          const double fnext = loss_scale_value(c, he[ZF_SLOT]), regnext = he[RX_SLOT];
          const double relnext = rel_from(he[NRM_SLOT]), nxnext = std::sqrt(he[NRM_SLOT + 1]);
          const double ftnext = tst ? loss_scale_value(c, he[TF_SLOT]) : nan;
          const bool stop = ndx < x_tol * std::max(nxcur, 1.0) || frel <= f_tol || pri < x_tol;
          if (stop && epoch != max_epoch)   // iterate.jl:235-247: stats of x_new
            push(fnext + regnext, fnext, pri, relnext, frel_of(fnext + regnext), now(), ftnext);
          fcur = fnext;
          ftcur = ftnext;
          regcur = regnext;
          relcur = relnext;
          nxcur = nxnext;
          ++epochs;
          if (stop) {
            if (enq > done) restore_last();   // the epoch enqueued past this one
            break;
          }
        }
        sync(c);
        c->lbfgs_pending = false;
        invalidate_caches(c);   // z, f and ∇q of the last enqueued point, which may be past the stop
        d2h(c, x_out, c->x, m);
        sync(c);
        *n_hist = nh;
        *epochs_out = epochs;
        if (c->timing) tresolve(c);
        return;
      }
      for (int64_t epoch = 1; epoch <= max_epoch; ++epoch) {
        double dt = now();
        // f(x): the z of x is cached (the previous step's ∇q(x_new) / the Newton step's forward)
        // except at epoch 1; its value is copied out of the deferred slot before the step's
        // forward at x_new reuses it
        if (c->loss == SCS_LOSS_ROSENBROCK) {
          HCK(launch_rosen(c->x, m, 0, c->scal + FX_SLOT, nullptr, 0, c->st));
        } else {
          forward(c, x, c->x, 0, false);
          HCK(hipMemcpyAsync(c->scal + FX_SLOT, c->scal + ZF_SLOT, sizeof(double), hipMemcpyDeviceToDevice, c->st));
        }
        HCK(launch_reg_value(prox_args(c), c->x, m, c->scal + RX_SLOT, c->scal + 64 + 2 * 256, c->st));
        if (tst) ftest_enqueue(c, c->x);   // -> scal[TF_SLOT], read back with the epoch's scalars
        hipEvent_t e0;
        tbegin(c, T_STEP, &e0);
        tag_slot(x_new).v = c->xtag_next++;   // the step writes x_new (c->xn)
        if (c->method == SCS_PROX_LQNSCORE)
          step_lqn(c, x, x_prev, epoch, x_new, nullptr, &pri);
        else
          step_newton(c, x, epoch, x_new, nullptr, &pri);
        tend(c, T_STEP, e0);
        HCK(launch_norms3(c->x, c->xstar, c->xn, m, c->scal + NRM_SLOT, c->scal + 64 + 3 * 256, c->st));
        d2h(c, hs, c->scal, LOOP_SLOTS);
        sync(c);
        lbfgs_settle(c, true);
        const double fval = loss_scale_value(c, hs[FX_SLOT]);
        const double obj = fval + hs[RX_SLOT];
        const double rel = rel_from(hs[NRM_SLOT]);
        const double frel = frel_of(obj);
        const double ft = tst ? loss_scale_value(c, hs[TF_SLOT]) : nan;
        push(obj, fval, pri, rel, frel, dt, ft);
        if (epoch == max_epoch) push(obj, fval, pri, rel, frel, now(), ft);   // iterate.jl:219-231
        pri = hs[0];
        const double nx = std::sqrt(hs[NRM_SLOT + 1]), ndx = std::sqrt(hs[NRM_SLOT + 2]);
        const bool stop = ndx < x_tol * std::max(nx, 1.0) || frel <= f_tol || pri < x_tol;
        if (stop && epoch != max_epoch) {   // iterate.jl:235-247: stats of x_new
          dt = now();
          double fv = eval_f_dev(c, x_new, c->xn);
          const double ob = fv + eval_reg_dev(c, c->xn);
          const double ft = tst ? eval_ftest_dev(c, x_new, c->xn) : nan;
          HCK(launch_norms3(c->xn, c->xstar, nullptr, m, c->scal + NRM_SLOT, c->scal + 64 + 3 * 256, c->st));
          d2h(c, hs + NRM_SLOT, c->scal + NRM_SLOT, 1);
          sync(c);
          push(ob, fv, pri, rel_from(hs[NRM_SLOT]), frel_of(ob), dt, ft);
        }
        // x_prev <- x, x <- x_new: rotate the device buffers and the host identities' tags
        std::swap(x_prev, x);
        tag_slot(x).v = tag_slot(x_new).v;
        double* t = c->xp;
        c->xp = c->x;
        c->x = c->xn;
        c->xn = t;
        ++epochs;
        if (stop) break;
      }
      d2h(c, x_out, c->x, m);
      sync(c);
      *n_hist = nh;
      *epochs_out = epochs;
      if (c->timing) tresolve(c);
      return;
    }
    for (int64_t epoch = 1; epoch <= max_epoch; ++epoch) {
      double dt = now();
      double fval = 0.0;
      double obj = fobj_of(x, &fval);
      double ft = ftest_of(x);
      double rel = rel_of(x);
      double frel = frel_of(obj);
      push(obj, fval, pri, rel, frel, dt, ft);
      for (int64_t i = 1; i <= iend; ++i) {   // for (i, sample) in enumerate(data) (iterate.jl:204-255)
        if (epoch == max_epoch && i == iend) {   // iterate.jl:219-231 (x as of this batch)
          dt = now();
          obj = fobj_of(x, &fval);
          ft = ftest_of(x);
          rel = rel_of(x);
          frel = frel_of(obj);
          push(obj, fval, pri, rel, frel, dt, ft);
        }
        hipEvent_t e0;
        tbegin(c, T_STEP, &e0);
        select_batch(c, nb > 0 ? i - 1 : -1);
        {
          BatchScope bs(c);
          const uint64_t tx = xtag_of(c, x), tp = xtag_of(c, x_prev);
          const size_t vb = sizeof(double) * m;
          if (nb == 0 && tp && tp == dev_x)   // x_prev = the previous step's x, still in c->x
            HCK(hipMemcpyAsync(c->xp, c->x, vb, hipMemcpyDeviceToDevice, c->st));
          else
            h2d(c, c->xp, x_prev, m);
          if (nb == 0 && tx && tx == dev_xn)
            HCK(hipMemcpyAsync(c->x, c->xn, vb, hipMemcpyDeviceToDevice, c->st));
          else
            h2d(c, c->x, x, m);
          dev_x = tx;
          tag_slot(x_new).v = c->xtag_next++;   // the step writes x_new
          if (c->method == SCS_PROX_LQNSCORE)
            step_lqn(c, x, x_prev, epoch, x_new, nullptr, &pri);
          else
            step_newton(c, x, epoch, x_new, nullptr, &pri);
          dev_xn = xtag_of(c, x_new);   // the step's tail wrote x_new to c->xn (and downloaded it)
        }
        unselect_view(c);
        tend(c, T_STEP, e0);
        const double nx = nrm(x, nullptr);
        const double ndx = nrm(x_new, x);
        last_nx = nx;     // the epoch-end test (:257) reads the same pair after the swap
        last_ndx = ndx;
        const bool stop = ndx < x_tol * std::max(nx, 1.0) || frel <= f_tol || pri < x_tol;
        if (stop && epoch != max_epoch) {   // iterate.jl:235-247 (f_rel_error is refreshed for the test at :257)
          dt = now();
          obj = fobj_of(x_new, &fval);
          ft = ftest_of(x_new);
          rel = rel_of(x_new);
          frel = frel_of(obj);
          push(obj, fval, pri, rel, frel, dt, ft);
        }
        std::swap(x_prev, x);
        std::memcpy(x, x_new, sizeof(double) * m);
        tag_slot(x).v = tag_slot(x_new).v;   // same content
        if (stop) {
          ++epochs;
          break;
        }
      }
      // ‖x − x_prev‖, ‖x_prev‖ = the last inner step's ‖x_new − x‖, ‖x‖ (same operands, same order)
      if (last_ndx < x_tol * std::max(last_nx, 1.0) || frel <= f_tol ||
          pri < x_tol)
        break;   // iterate.jl:257-259
      ++epochs;
    }
    std::memcpy(x_out, x, sizeof(double) * m);
    *n_hist = nh;
    *epochs_out = epochs;
    if (c->timing) tresolve(c);
  });
}

int scs_smoother_eval(scs_ctx* c, const double* x, double* gr, double* Hr) {
  if (is_group(c)) return scs_smoother_eval(c->subs[0], x, gr, Hr);   // m-space, no exchange
  return guarded(c, [&] {
    if (!c->smooth_set) fail(c, SCS_ERR_STATE, "no smoother");
    h2d(c, c->xn, x, c->m);
    HCK(launch_smoother(c->smooth, c->xn, c->m, c->mu, c->slb, c->sub, c->wel, c->gr, c->Hr, c->st));
    d2h(c, gr, c->gr, c->m);
    d2h(c, Hr, c->Hr, c->m);
    sync(c);
  });
}

int scs_prox_eval(scs_ctx* c, const double* z, const double* Hr, double lam, double alpha, double* out) {
  if (is_group(c)) return scs_prox_eval(c->subs[0], z, Hr, lam, alpha, out);
  return guarded(c, [&] {
    if (!c->reg_set) fail(c, SCS_ERR_STATE, "no regularizer");
    h2d(c, c->zb, z, c->m);
    h2d(c, c->Hr, Hr, c->m);
    ProxArgsH P = prox_args(c);
    P.lam = lam;
    HCK(launch_prox_only(P, c->zb, c->Hr, alpha, c->m, c->hinv, c->xn, c->st));
    d2h(c, out, c->xn, c->m);
    sync(c);
  });
}

int scs_gram_eval(scs_ctx* c, const double* w, double* G, int64_t ldg) {
  return guarded(c, [&] {
    refuse_multi(c, "scs_gram_eval (scs_multi_products_eval / scs_multi_system_eval serve it)");
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    std::vector<double> wp(c->Npad, 0.0);
    std::memcpy(wp.data(), w, sizeof(double) * c->N);
    h2d(c, c->wN, wp.data(), c->Npad);
    ensure_gram(c);
    hipEvent_t e0;
    tbegin(c, T_GRAM, &e0);
    gram_main(c, c->wN, c->G, 0);
    tend(c, T_GRAM, e0);
    HCK(launch_symmetrize(c->G, c->mpad, c->m, c->st));
    HCK(hipMemcpy2DAsync(G, sizeof(double) * ldg, c->G, sizeof(double) * c->mpad, sizeof(double) * c->m, c->m,
                         hipMemcpyDeviceToHost, c->st));
    sync(c);
    if (c->timing) tresolve(c);
  });
}

// P = A diag(h) Aᵀ of the selected batch or the full data, by the path a ProxGGNSCORE step takes: from
// the nonzeros (scs_set_sparse_sample on a sparse A), else the Aᵀ copy (of the mirror) on the MFMA tiles
int scs_sample_gram_eval(scs_ctx* c, const double* h, double* P, int64_t ldp) {
  return guarded(c, [&] {
    refuse_multi(c, "scs_sample_gram_eval (scs_multi_products_eval / scs_multi_system_eval serve it)");
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    if (sharded(c)) fail(c, SCS_ERR_ARG, "scs_sample_gram_eval runs on one rank");
    if (!h || !P) fail(c, SCS_ERR_ARG, "scs_sample_gram_eval: null argument");
    HCK(hipSetDevice(c->dev));
    BatchScope scope(c);
    const int64_t N = c->N, m = c->m;
    if (ldp < N) fail(c, SCS_ERR_ARG, "scs_sample_gram_eval: ldp %lld < N %lld", (long long)ldp, (long long)N);
    const bool sps = sparse_sample_path(c);
    const int64_t NpS = round_up(N, 128);
    std::vector<double> hp(c->mpad, 0.0);
    std::memcpy(hp.data(), h, sizeof(double) * m);
    double* hd = dalloc<double>(c, c->mpad, false);
    double *Ps = nullptr, *Pown = nullptr, *At = nullptr;   // Ps: the size's kept set, or Pown
    int2* tiles = nullptr;
    struct Free {
      scs_ctx* c;
      double **a, **b, **d;
      int2** t;
      ~Free() {
        (void)hipStreamSynchronize(c->st);
        dfree_t(c, *a);
        dfree_t(c, *b);
        dfree_t(c, *d);
        dfree_t(c, *t);
      }
    } fr{c, &hd, &Pown, &At, &tiles};
    h2d(c, hd, hp.data(), c->mpad);
    if (sps) {
      Ps = sample_sys(c, N).Ps;
    } else {
      Ps = Pown = dalloc<double>(c, (size_t)NpS * NpS);
    }
    hipEvent_t e0;
    if (sps) {
      tbegin(c, T_GRAM, &e0);
      sparse_sample_gram(c, hd, Ps, NpS);
      tend(c, T_GRAM, e0);
    } else {
      const double* A = dense_A(c);
      At = dalloc<double>(c, (size_t)NpS * c->mpad);
      HCK(launch_transpose(A, dense_a32(c), c->Npad, N, m, At, c->mpad, NpS, c->st));
      const int nb = (int)(NpS / 128);
      std::vector<int2> tl((size_t)nb * (nb + 1) / 2 + 1);
      int nt = 0;
      gram_tile_list(nb, tl.data(), &nt);
      tiles = dalloc<int2>(c, std::max(nt, 1));
      HCK(hipMemcpyAsync(tiles, tl.data(), sizeof(int2) * nt, hipMemcpyHostToDevice, c->st));
      tbegin(c, T_GRAM, &e0);
      HCK(gram_launch_gen(At, c->mpad, At, c->mpad, hd, 0, c->mpad, tiles, nt, Ps, NpS, /*GRAM_UPPER*/ 4, c->st));
      tend(c, T_GRAM, e0);
    }
    HCK(launch_symmetrize(Ps, NpS, N, c->st));
    if (N > 0)
      HCK(hipMemcpy2DAsync(P, sizeof(double) * ldp, Ps, sizeof(double) * NpS, sizeof(double) * N, N,
                           hipMemcpyDeviceToHost, c->st));
    sync(c);
    if (c->timing) tresolve(c);
  });
}

// the sample-space system of a single-output ProxGGNSCORE step at x, of the selected batch or the full
// data: the smoother, then the function the step calls (ggn_sample_system: its cached Aᵀ / tile list /
// scratch, or P from the nonzeros), before the solve.  M of order n1 = N + 1 and b
int scs_sample_system_eval(scs_ctx* c, const double* x, double* M, int64_t ldm, double* b) {
  return guarded(c, [&] {
    if (multi(c))
      fail(c, SCS_ERR_STATE, "scs_sample_system_eval takes a single-output context: this one has nout = %d "
                             "(scs_multi_sample_system_eval serves it)", c->nout);
    if (!c->loss_set) fail(c, SCS_ERR_STATE, "no loss: call scs_set_loss first");
    if (c->loss == SCS_LOSS_CALLBACK)
      fail(c, SCS_ERR_ARG, "scs_sample_system_eval: a callback loss brings its own J (the system of the caller's "
                           "rows is not the data's)");
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    if (!c->reg_set || !c->smooth_set)
      fail(c, SCS_ERR_STATE, "scs_sample_system_eval needs the regularizer and the smoother (h = 1 ./ Hr, λ gr)");
    if (sharded(c)) fail(c, SCS_ERR_ARG, "scs_sample_system_eval runs on one rank");
    if (c->ggn == SCS_GGN_NONE) fail(c, SCS_ERR_ARG, "scs_sample_system_eval needs an out_fn / GGN loss kind");
    HCK(hipSetDevice(c->dev));
    BatchScope scope(c);
    const int64_t N = c->N, n1 = N + 1;
    // (a sparse view built for ProxLQNSCORE's products holds neither the CSR rows nor a sample-space copy)
    if (c->spview >= 0 && !sparse_sample_path(c))
      fail(c, SCS_ERR_STATE, "scs_sample_system_eval: the selected batch is held as a sparse view of ProxLQNSCORE's "
                             "products (scs_set_sparse_batches), which keeps no rows for the sample-space system");
    if (c->Nglob + 1 > c->m)
      fail(c, SCS_ERR_ARG, "scs_sample_system_eval: N + 1 = %lld > m = %lld is the feature branch's shape "
                           "(scs_solve_eval / scs_gram_eval serve it)", (long long)(c->Nglob + 1), (long long)c->m);
    if (!x) fail(c, SCS_ERR_ARG, "scs_sample_system_eval: null x");
    if (M && ldm < n1)
      fail(c, SCS_ERR_ARG, "scs_sample_system_eval: ldm %lld < N + 1 = %lld", (long long)ldm, (long long)n1);
    invalidate_caches(c);
    h2d(c, c->x, x, c->m);
    HCK(launch_smoother(c->smooth, c->x, c->m, c->mu, c->slb, c->sub, c->wel, c->gr, c->Hr, c->st));
    const SampleSys& S = ggn_sample_system(c, x);
    // Ms is row-major: its transpose lands column-major on the host through a column-major staging copy
    if (M) {
      double* T = dalloc<double>(c, (size_t)S.n1pad * S.n1pad, false);
      struct Free {
        scs_ctx* c;
        double** p;
        ~Free() {
          (void)hipStreamSynchronize(c->st);
          dfree_t(c, *p);
        }
      } fr{c, &T};
      HCK(qr_from_rowmajor(S.Ms, S.n1pad, T, S.n1pad, n1, S.n1pad, c->st));
      HCK(hipMemcpy2DAsync(M, sizeof(double) * ldm, T, sizeof(double) * S.n1pad, sizeof(double) * n1, n1,
                           hipMemcpyDeviceToHost, c->st));
      sync(c);
    }
    if (b) d2h(c, b, S.bS, n1);
    sync(c);
    invalidate_caches(c);
    if (c->timing) tresolve(c);
  });
}

// The m x m system of ProxNSCORE / ProxGGNSCORE from given weights: (Aᵀ diag(w) A + diag(dvec)) x = rhs,
// through the production path (Gram, then solve_system: Cholesky with the LU fallback, or the LU
// alone with mode 1).  G is the step's scratch, so nothing else changes.
int scs_solve_eval(scs_ctx* c, const double* w, const double* dvec, const double* rhs, int mode, double* x,
                   int* used_lu) {
  return guarded(c, [&] {
    refuse_multi(c, "scs_solve_eval (scs_multi_products_eval / scs_multi_system_eval serve it)");
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    if (c->nranks > 1) fail(c, SCS_ERR_ARG, "scs_solve_eval runs on one rank");
    if (!w || !dvec || !rhs || !x) fail(c, SCS_ERR_ARG, "scs_solve_eval: null argument");
    HCK(hipSetDevice(c->dev));
    std::vector<double> wp(c->Npad, 0.0), v(c->mpad, 0.0);
    std::memcpy(wp.data(), w, sizeof(double) * c->N);
    h2d(c, c->wN, wp.data(), c->Npad);
    ensure_gram(c);
    hipEvent_t e0;
    tbegin(c, T_GRAM, &e0);
    gram_main(c, c->wN, c->G, 0);
    tend(c, T_GRAM, e0);
    std::memcpy(v.data(), dvec, sizeof(double) * c->m);
    h2d(c, c->gtmp2, v.data(), c->mpad);
    HCK(launch_diag_add(c->G, c->mpad, c->m, 1.0, c->gtmp2, c->st));
    std::memcpy(v.data(), rhs, sizeof(double) * c->m);
    h2d(c, c->gq, v.data(), c->mpad);
    sync(c);
    c->g_from_cache = false;
    if (mode < 0 || mode > 2) fail(c, SCS_ERR_ARG, "scs_solve_eval: mode %d (0 step path, 1 LU, 2 QR)", mode);
    solve_system(c, c->gq, mode == 1, mode == 2);
    d2h(c, x, c->gq, c->m);
    sync(c);
    if (used_lu) *used_lu = c->lu_fallback_used ? 1 : 0;
    invalidate_caches(c);
    if (c->timing) tresolve(c);
  });
}

// A x = b for a host row-major n x n A by the hand-written LU (getrf + getrs semantics); ipiv
// (0-based, LAPACK order) and info (first zero pivot, 1-based) as dgetrf reports them.  Needs a
// context only (no data).
int scs_lu_eval(scs_ctx* c, int64_t n, const double* A, const double* b, double* x, int32_t* ipiv, int* info) {
  return guarded(c, [&] {
    if (n < 1 || !A || !b || !x) fail(c, SCS_ERR_ARG, "scs_lu_eval: bad arguments");
    HCK(hipSetDevice(c->dev));
    const int64_t np = round_up(n, 128);
    if (c->lu_np != np) {
      if (c->luM) dfree_t(c, c->luM);
      if (c->lub) dfree_t(c, c->lub);
      if (c->luinfo) dfree_t(c, c->luinfo);
      c->luM = dalloc<double>(c, (size_t)np * np);
      c->lub = dalloc<double>(c, np);
      c->luinfo = dalloc<int>(c, 1);
      c->lu_np = np;
    }
    double* M = c->luM;
    double* bb = c->lub;
    auto upload = [&] {   // (also the system of a column-step redo, lu_factor_checked)
      HCK(hipMemsetAsync(M, 0, sizeof(double) * np * np, c->st));
      HCK(hipMemsetAsync(bb, 0, sizeof(double) * np, c->st));
      HCK(hipMemcpy2DAsync(M, sizeof(double) * np, A, sizeof(double) * n, sizeof(double) * n, n,
                           hipMemcpyHostToDevice, c->st));
      HCK(hipMemcpyAsync(bb, b, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
    };
    upload();
    HCK(lu_aux_init(&c->lu, np, c->st));
    hipEvent_t e0;
    tbegin(c, T_SOLVE, &e0);
    const int hinfo = lu_factor_checked(c, M, np, n, np, c->luinfo, upload);
    if (hinfo == 0) HCK(lu_solve(M, np, np, &c->lu, bb, c->st));
    tend(c, T_SOLVE, e0);
    // x only without a zero pivot; ipiv whenever the factorization completed -- dgetrf's pivots with
    // info > 0 too (the header's contract)
    if (hinfo == 0) HCK(hipMemcpyAsync(x, bb, sizeof(double) * n, hipMemcpyDeviceToHost, c->st));
    if (ipiv) HCK(hipMemcpyAsync(ipiv, c->lu.ipiv, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->st));
    sync(c);
    if (info) *info = hinfo;
    if (c->timing) tresolve(c);
  });
}

// M x = b for a host symmetric positive definite M by the hand-written Cholesky, on buffers of its
// own through the step's sequence (chol_factor_checked, chol_solve_checked): M and U column-major
// n x n, upper triangles.  Needs a context only (no data).
int scs_chol_eval(scs_ctx* c, int64_t n, const double* M, const double* b, double* x, double* U, int* info) {
  return guarded(c, [&] {
    if (n < 1 || !M || !b || !x) fail(c, SCS_ERR_ARG, "scs_chol_eval: bad arguments");
    HCK(hipSetDevice(c->dev));
    const int64_t np = round_up(n, 128);
    if (c->ce_np != np) {
      for (double** p : {&c->ceG, &c->ceW, &c->cey, &c->cerbk, &c->ceb}) dfree_t(c, *p);
      dfree_t(c, c->cetri);
      dfree_t(c, c->ceinfo);
      chol_aux_free(&c->ceaux);
      c->ce_np = 0;
      const int nb = (int)(np / 128);
      c->ceG = dalloc<double>(c, (size_t)np * np);
      c->ceW = dalloc<double>(c, (size_t)np * 128);
      c->cey = dalloc<double>(c, np);
      c->cerbk = dalloc<double>(c, np);
      c->ceb = dalloc<double>(c, np);
      c->ceinfo = dalloc<int>(c, 1);
      std::vector<int2> tr((size_t)nb * (nb + 1) / 2);
      gram_tile_list_rowmajor(nb, tr.data());
      c->cetri = dalloc<int2>(c, tr.size());
      HCK(hipMemcpyAsync(c->cetri, tr.data(), sizeof(int2) * tr.size(), hipMemcpyHostToDevice, c->st));
      HCK(chol_aux_init(&c->ceaux, np, c->st));   // (drains the stream: tr stays valid)
      c->ce_np = np;
    }
    const CholSys s = {c->ceG, n, np, c->ceW, &c->ceaux, c->cetri, c->cey, c->cerbk, c->ceinfo};
    double* bb = c->ceb;
    auto upload = [&] {   // (also the system of a redo after a late chain wait, chol_factor_checked)
      HCK(hipMemsetAsync(s.G, 0, sizeof(double) * np * np, c->st));
      HCK(hipMemcpy2DAsync(s.G, sizeof(double) * np, M, sizeof(double) * n, sizeof(double) * n, n,
                           hipMemcpyHostToDevice, c->st));
      HCK(chol_diag_pad(s.G, np, n, np, c->st));
    };
    upload();
    HCK(hipMemsetAsync(bb, 0, sizeof(double) * np, c->st));
    HCK(hipMemcpyAsync(bb, b, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
    hipEvent_t e0;
    tbegin(c, T_SOLVE, &e0);
    const int hinfo = chol_factor_checked(c, s, upload);
    if (hinfo == 0) chol_solve_checked(c, s, bb);
    tend(c, T_SOLVE, e0);
    if (hinfo == 0) HCK(hipMemcpyAsync(x, bb, sizeof(double) * n, hipMemcpyDeviceToHost, c->st));
    if (U)
      HCK(hipMemcpy2DAsync(U, sizeof(double) * n, s.G, sizeof(double) * np, sizeof(double) * n, n,
                           hipMemcpyDeviceToHost, c->st));
    sync(c);
    if (info) *info = hinfo;
    if (c->timing) tresolve(c);
  });
}

// A x = b for a host row-major n x n A by the Householder QR, on buffers of its own through the
// sample-space step's sequence (qr_from_rowmajor, qr_run); R column-major n x n, its upper triangle.
// Needs a context only (no data).
int scs_qr_eval(scs_ctx* c, int64_t n, const double* A, const double* b, double* x, double* R) {
  return guarded(c, [&] {
    if (n < 1 || !A || !b || !x) fail(c, SCS_ERR_ARG, "scs_qr_eval: bad arguments");
    HCK(hipSetDevice(c->dev));
    const int64_t np = round_up(n, 128);
    if (c->qe_np != np) {
      for (double** p : {&c->qeS, &c->qeA, &c->qeb}) dfree_t(c, *p);
      c->qeS = dalloc<double>(c, (size_t)np * np);
      c->qeA = dalloc<double>(c, (size_t)np * np);
      c->qeb = dalloc<double>(c, np);
      c->qe_np = np;
    }
    HCK(hipMemcpyAsync(c->qeS, A, sizeof(double) * n * n, hipMemcpyHostToDevice, c->st));
    HCK(qr_from_rowmajor(c->qeS, n, c->qeA, np, n, np, c->st));
    HCK(hipMemsetAsync(c->qeb, 0, sizeof(double) * np, c->st));
    HCK(hipMemcpyAsync(c->qeb, b, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
    hipEvent_t e0;
    tbegin(c, T_SOLVE, &e0);
    qr_run(c, &c->qre, c->qebk, c->qebk_n, c->qeA, np, c->qeb);
    tend(c, T_SOLVE, e0);
    HCK(hipMemcpyAsync(x, c->qeb, sizeof(double) * n, hipMemcpyDeviceToHost, c->st));
    if (R)
      HCK(hipMemcpy2DAsync(R, sizeof(double) * n, c->qeA, sizeof(double) * np, sizeof(double) * n, n,
                           hipMemcpyDeviceToHost, c->st));
    sync(c);
    if (c->timing) tresolve(c);
  });
}

// Columns cols[0..ncols) of the local A, column-major N x ncols (ld = N).
int scs_get_columns(scs_ctx* c, const int64_t* cols, int64_t ncols, double* out) {
  return guarded(c, [&] {
    if (!c->has_data || c->generic || c->sparse) fail(c, SCS_ERR_STATE, "scs_get_columns needs a dense A");
    for (int64_t k = 0; k < ncols; ++k)
      if (cols[k] < 0 || cols[k] >= c->dc) fail(c, SCS_ERR_ARG, "column %lld out of range", (long long)cols[k]);
    HCK(hipSetDevice(c->dev));
    int64_t* dc = dalloc<int64_t>(c, ncols);
    double* dout = dalloc<double>(c, (size_t)ncols * c->N);
    HCK(hipMemcpyAsync(dc, cols, sizeof(int64_t) * ncols, hipMemcpyHostToDevice, c->st));
    HCK(launch_get_columns(c->A, c->a32, c->nstage, dc, ncols, c->N, dout, c->st));
    HCK(hipMemcpyAsync(out, dout, sizeof(double) * ncols * c->N, hipMemcpyDeviceToHost, c->st));
    sync(c);
    dfree_t(c, dc);
    dfree_t(c, dout);
  });
}

// The production Gram launch with weights w and -- where the step fuses it (256 x 128 tiles) --
// Aᵀv in the same pass: entries G(i_k, j_k) (ij = n pairs, 0-based) and Aᵀv (m) to the host.
int scs_gram_atv_eval(scs_ctx* c, const double* w, const double* v, const int64_t* ij, int64_t n, double* gvals,
                      double* atv, int* fused) {
  return guarded(c, [&] {
    refuse_multi(c, "scs_gram_atv_eval (scs_multi_products_eval / scs_multi_system_eval serve it)");
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    if (n < 0 || (n > 0 && (!ij || !gvals))) fail(c, SCS_ERR_ARG, "scs_gram_atv_eval: bad sample list");
    HCK(hipSetDevice(c->dev));
    std::vector<double> wp(c->Npad, 0.0);
    std::memcpy(wp.data(), w, sizeof(double) * c->N);
    h2d(c, c->wN, wp.data(), c->Npad);
    std::memcpy(wp.data(), v, sizeof(double) * c->N);
    h2d(c, c->vN, wp.data(), c->Npad);
    ensure_gram(c);
    const bool fuse = gram_fuse_ok(c->tall) != 0 && !c->sparse;
    hipEvent_t e0;
    tbegin(c, T_GRAM, &e0);
    gram_main(c, c->wN, c->G, 0, fuse ? c->vN : nullptr, c->gtmp);
    tend(c, T_GRAM, e0);
    if (!fuse) gemv_t_local(c, c->vN, c->gtmp);
    std::vector<int2> hij((size_t)std::max<int64_t>(n, 1));
    for (int64_t k = 0; k < n; ++k) {
      const int64_t i = ij[2 * k], j = ij[2 * k + 1];
      if (i < 0 || j < 0 || i >= c->m || j >= c->m) fail(c, SCS_ERR_ARG, "sample %lld out of range", (long long)k);
      hij[k] = make_int2((int)std::min(i, j), (int)std::max(i, j));   // the upper triangle holds G
    }
    int2* dij = dalloc<int2>(c, hij.size());
    double* dv = dalloc<double>(c, hij.size());
    HCK(hipMemcpyAsync(dij, hij.data(), sizeof(int2) * n, hipMemcpyHostToDevice, c->st));
    HCK(launch_gather_entries(c->G, c->mpad, dij, (int)n, dv, c->st));
    if (n > 0) d2h(c, gvals, dv, n);
    if (atv) d2h(c, atv, c->gtmp, c->m);
    sync(c);
    dfree_t(c, dij);
    dfree_t(c, dv);
    if (fused) *fused = fuse ? 1 : 0;
    invalidate_caches(c);
    if (c->timing) tresolve(c);
  });
}

int scs_gemv_t_eval(scs_ctx* c, const double* v, double* out) {
  return guarded(c, [&] {
    refuse_multi(c, "scs_gemv_t_eval (scs_multi_products_eval / scs_multi_system_eval serve it)");
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    std::vector<double> vp(c->Npad, 0.0);
    std::memcpy(vp.data(), v, sizeof(double) * c->N);
    h2d(c, c->vN, vp.data(), c->Npad);
    matvec_t(c, c->vN, c->gtmp);
    d2h(c, out, c->gtmp, c->m);
    sync(c);
  });
}

int scs_gemv_n_eval(scs_ctx* c, const double* x, double* out) {
  return guarded(c, [&] {
    refuse_multi(c, "scs_gemv_n_eval (scs_multi_products_eval / scs_multi_system_eval serve it)");
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    h2d(c, c->xn, x, c->m);
    const int ns = matvec_n(c, c->xn, c->nsplit);
    HCK(launch_epilogue(c->loss ? c->loss : SCS_LOSS_LEAST_SQUARES, SCS_GGN_NONE, EPI_Z, c->zpart, ns, c->Npad,
                        c->y, c->N, c->Npad, 1.0, c->z, nullptr, nullptr, nullptr, nullptr, c->valpart, c->st));
    d2h(c, out, c->z, c->N);
    sync(c);
    c->zvalid = false;
  });
}

// ---- multi-output targets -------------------------------------------------------------------
int scs_set_outputs(scs_ctx* c, int nout) {
  if (!c) return SCS_ERR_ARG;
  if (is_group(c)) {
    c->err = "scs_set_outputs takes a single-device context (scs_create): a multi-device context (devices=[...]) is "
             "not supported with nout";
    return SCS_ERR_ARG;
  }
  return guarded(c, [&] {
    if (nout != 0 && (nout < 2 || nout > 16))
      fail(c, SCS_ERR_ARG, "scs_set_outputs: nout = %d is outside 2..16 (0 clears the mode)", nout);
    if (nout && c->nranks > 1) fail(c, SCS_ERR_ARG, "nranks > 1 is not supported with scs_set_outputs (nout = %d)", nout);
    if (nout == c->nout) return;
    HCK(hipSetDevice(c->dev));
    if (c->has_data) {   // the dimensions change meaning: the data goes, as with a new data door
      sync(c);
      reset_data(c);
    }
    c->loss_set = false;
    c->nout = nout;
  });
}

int scs_get_outputs(scs_ctx* c, int* nout, int64_t* nvar) {
  if (!c) return SCS_ERR_ARG;
  if (is_group(c)) {
    if (nout) *nout = 1;
    if (nvar) *nvar = c->grpm;
    return SCS_OK;
  }
  return guarded(c, [&] {
    if (nout) *nout = kout(c);
    if (nvar) *nvar = c->m;
  });
}

// The mode of a sparse A under scs_set_outputs: stored without effect while nout is unset; with nout
// set the sparse doors accept A and the products run with K right-hand sides (multi_sparse.hip).
int scs_set_sparse_outputs(scs_ctx* c, int on) {
  if (!c) return SCS_ERR_ARG;
  if (is_group(c)) {
    c->err = "scs_set_sparse_outputs takes a single-device context (scs_create): a multi-device context "
             "(devices=[...]) is not supported with nout";
    return SCS_ERR_ARG;
  }
  return guarded(c, [&] { c->sparse_outputs = on ? 1 : 0; });
}

// ProxGGNSCORE's sample-space branch with nout set (N·nout + 1 <= d·nout, a dense A): stored without
// effect while nout is unset.  Switching it off with the data in place gives the branch's buffers back.
int scs_set_multi_sample(scs_ctx* c, int on) {
  if (!c) return SCS_ERR_ARG;
  if (is_group(c)) {
    c->err = "scs_set_multi_sample takes a single-device context (scs_create): a multi-device context "
             "(devices=[...]) is not supported with nout";
    return SCS_ERR_ARG;
  }
  return guarded(c, [&] {
    const int v = on ? 1 : 0;
    if (v == c->multi_sample) return;
    c->multi_sample = v;
    if (!v && multi(c) && c->has_data) {   // the view in place (a dense A) and every pooled batch view
      HCK(hipSetDevice(c->dev));
      sync(c);
      auto give_back = [c](ViewData& w) {
        if (!w.At) return;
        free_buffers(c, w, VB_SAMPLE);
        static_cast<ViewSample&>(w) = ViewSample();
      };
      if (!c->sparse) give_back(*c);
      for (NView& w : c->bpool) give_back(w);
    }
  });
}

// Minibatches with nout set (a dense A): stored without effect while nout is unset.  Changing it drops
// the pooled batch views; switching it off with a list registered on a multi-output context clears the list.
int scs_set_multi_batches(scs_ctx* c, int on) {
  if (!c) return SCS_ERR_ARG;
  if (is_group(c)) {
    c->err = "scs_set_multi_batches takes a single-device context (scs_create): a multi-device context "
             "(devices=[...]) is not supported with nout";
    return SCS_ERR_ARG;
  }
  return guarded(c, [&] {
    const int v = on ? 1 : 0;
    if (v == c->multi_batches) return;
    HCK(hipSetDevice(c->dev));
    sync(c);
    c->multi_batches = v;
    if (!v && multi(c) && !c->boff.empty()) {
      clear_batches(c);
    } else {
      free_dense_views(c);   // the pooled views go, the registered list stays
      free_sparse_views(c);
      if (c->bsel >= 0) select_batch(c, c->bsel);
    }
    invalidate_caches(c);
    sync(c);
  });
}

// Minibatches with nout set on a sparse A (scs_set_sparse_outputs): lifts scs_set_batches' dense-A
// requirement; scs_set_multi_batches stays the gate.  Stored without effect while nout is unset or on a
// dense A.  Changing it drops the pooled batch views; switching it off with a list registered on a sparse
// multi-output context clears the list.
int scs_set_multi_sparse_batches(scs_ctx* c, int on) {
  if (!c) return SCS_ERR_ARG;
  if (is_group(c)) {
    c->err = "scs_set_multi_sparse_batches takes a single-device context (scs_create): a multi-device context "
             "(devices=[...]) is not supported with nout";
    return SCS_ERR_ARG;
  }
  return guarded(c, [&] {
    const int v = on ? 1 : 0;
    if (v == c->multi_sparse_batches) return;
    HCK(hipSetDevice(c->dev));
    sync(c);
    c->multi_sparse_batches = v;
    if (!v && multi(c) && c->sparse && !c->boff.empty()) {
      clear_batches(c);
    } else {
      free_dense_views(c);   // the pooled views go, the registered list stays
      free_sparse_views(c);
      if (c->bsel >= 0) select_batch(c, c->bsel);
    }
    invalidate_caches(c);
    sync(c);
  });
}

// Batch b of the registered list as scs_select_batch gathers it: its n_b x d rows widened to fp64
// (column-major, leading dimension lda) and its n_b (x nout) targets.  The selection is left as found.
int scs_get_batch_data(scs_ctx* c, int64_t b, double* A_out, int64_t lda, double* Y_out) {
  if (!c) return SCS_ERR_ARG;
  if (is_group(c)) {
    c->err = "scs_get_batch_data takes a single-device context (scs_create)";
    return SCS_ERR_ARG;
  }
  return guarded(c, [&] {
    const int64_t nb = c->boff.empty() ? 0 : (int64_t)c->boff.size() - 1;
    if (b < 0 || b >= nb) fail(c, SCS_ERR_ARG, "scs_get_batch_data: batch %lld of %lld", (long long)b, (long long)nb);
    const int64_t n = c->boff[b + 1] - c->boff[b];
    if (A_out && lda < n) fail(c, SCS_ERR_ARG, "scs_get_batch_data: lda %lld < n_b %lld", (long long)lda, (long long)n);
    HCK(hipSetDevice(c->dev));
    const int64_t was = c->bsel;
    struct Restore {   // the caller's selection comes back even when the read fails
      scs_ctx* c;
      int64_t was;
      ~Restore() {
        try {
          select_batch(c, was);
          (void)hipStreamSynchronize(c->st);
        } catch (...) {
          unselect_view(c);
          c->bsel = -1;
        }
      }
    } restore{c, was};
    // a sparse multi-output context (scs_set_multi_sparse_batches): the batch's densified view whatever
    // kind the method asks for; a pool view made for this read alone goes with it
    const bool msb = multi(c) && c->sparse;
    const size_t npool = c->bpool.size();
    struct DropView {
      scs_ctx* c;
      size_t npool;
      ~DropView() {
        if (c->bpool.size() <= npool) return;
        (void)hipStreamSynchronize(c->st);
        free_view(c, c->bpool.back());
        c->bpool.pop_back();
        c->bheld.pop_back();
        c->bview = -1;
      }
    } drop{c, msb ? npool : (size_t)-1};
    select_batch(c, b, msb);
    if (c->spview >= 0) fail(c, SCS_ERR_ARG, "scs_get_batch_data: batch %lld is held as a sparse view", (long long)b);
    {
      BatchScope bs(c);
      read_rows(c, 0, c->N, A_out, lda, Y_out);
    }
  });
}

// A X (N x K) and Aᵀ V (d x K) of host operands through multi.hip's kernels; K is the call's own.  A
// sparse A held in the scs_set_sparse_outputs mode: through the context's own product arm, K = nout.
int scs_multi_products_eval(scs_ctx* c, int K, const double* X, const double* V, double* AX, double* ATV) {
  return guarded(c, [&] {
    if (!c->has_data || c->generic || (c->sparse && !multi(c)))
      fail(c, SCS_ERR_STATE, "scs_multi_products_eval needs a dense A");
    if (K < 1 || K > 16) fail(c, SCS_ERR_ARG, "scs_multi_products_eval: K = %d is outside 1..16", K);
    if ((X == nullptr) != (AX == nullptr) || (V == nullptr) != (ATV == nullptr))
      fail(c, SCS_ERR_ARG, "scs_multi_products_eval: X goes with AX and V with ATV");
    HCK(hipSetDevice(c->dev));
    // a selected sparse batch view (scs_set_multi_sparse_batches) takes the data's place: V is n_b x K
    std::unique_ptr<BatchScope> bs;
    if (multi(c) && c->spview >= 0) bs.reset(new BatchScope(c));
    const int64_t N = c->N, Npad = c->Npad, d = c->dc, dcp = c->dcp;
    if (c->sparse) {   // the step's own matvec_n / matvec_t on the context's workspace
      if (K != c->nout)
        fail(c, SCS_ERR_ARG, "scs_multi_products_eval: a sparse A takes K = nout = %d (the blocked copies are cut "
                             "for it), not K = %d", c->nout, K);
      invalidate_caches(c);
      if (X) {
        double* Z = dalloc<double>(c, (size_t)K * Npad);
        h2d(c, c->xn, X, d * K);
        const int ns = matvec_n(c, c->xn, c->nsplit);
        HCK(launch_multi_epilogue(SCS_LOSS_MULTI_LS, EPI_Z, K, c->zpart, ns, nullptr, N, Npad, 1.0, Z, nullptr, nullptr,
                                  nullptr, nullptr, c->st));
        if (N > 0)
          HCK(hipMemcpy2DAsync(AX, sizeof(double) * N, Z, sizeof(double) * Npad, sizeof(double) * N, K,
                               hipMemcpyDeviceToHost, c->st));
        sync(c);
        dfree_t(c, Z);
      }
      if (V) {
        double* dV = dalloc<double>(c, (size_t)Npad * K);   // zeroed: rows N..Npad stay zero
        if (N > 0)
          HCK(hipMemcpy2DAsync(dV, sizeof(double) * Npad, V, sizeof(double) * N, sizeof(double) * N, K,
                               hipMemcpyHostToDevice, c->st));
        matvec_t(c, dV, c->gtmp2);
        d2h(c, ATV, c->gtmp2, d * K);
        sync(c);
        dfree_t(c, dV);
      }
      return;
    }
    if (X) {
      const int ns = gemv_n_splits(Npad, d);
      double* dX = dalloc<double>(c, (size_t)d * K);
      double* Xt = dalloc<double>(c, (size_t)dcp * K);
      double* part = dalloc<double>(c, (size_t)ns * K * Npad);
      double* Z = dalloc<double>(c, (size_t)K * Npad);
      h2d(c, dX, X, d * K);
      HCK(launch_multi_pack_x(dX, d, dcp, K, Xt, c->st));
      HCK(launch_multi_ax(c->A, c->a32, c->nstage, Npad, dcp, K, Xt, ns, part, c->st));
      HCK(launch_multi_epilogue(SCS_LOSS_MULTI_LS, EPI_Z, K, part, ns, nullptr, N, Npad, 1.0, Z, nullptr, nullptr, nullptr,
                                nullptr, c->st));
      if (N > 0)
        HCK(hipMemcpy2DAsync(AX, sizeof(double) * N, Z, sizeof(double) * Npad, sizeof(double) * N, K,
                             hipMemcpyDeviceToHost, c->st));
      sync(c);
      for (double** q : {&dX, &Xt, &part, &Z}) dfree_t(c, *q);
    }
    if (V) {
      const int nch = multi_atv_chunks(Npad);
      double* dV = dalloc<double>(c, (size_t)Npad * K);   // zeroed: rows N..Npad stay zero
      double* part = dalloc<double>(c, (size_t)nch * K * dcp);
      double* out = dalloc<double>(c, (size_t)d * K);
      if (N > 0)
        HCK(hipMemcpy2DAsync(dV, sizeof(double) * Npad, V, sizeof(double) * N, sizeof(double) * N, K,
                             hipMemcpyHostToDevice, c->st));
      double* Vt = multi_vt(c, Npad * K);
      HCK(launch_multi_pack_v(dV, Npad, Npad, K, Vt, c->st));
      HCK(launch_multi_atv(c->A, c->a32, c->nstage, Npad, d, dcp, K, Vt, part, c->st));
      HCK(launch_multi_atv_finalize(part, nch, K, dcp, d, out, c->st));
      d2h(c, ATV, out, d * K);
      sync(c);
      for (double** q : {&dV, &part, &out}) dfree_t(c, *q);
    }
  });
}

// the assembled JᵀQJ (before λ diag Hr), vec(AᵀR) and f at x, by the step's own path
int scs_multi_system_eval(scs_ctx* c, const double* x, double* G, int64_t ldg, double* g, double* f) {
  return guarded(c, [&] {
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    if (!multi(c)) fail(c, SCS_ERR_STATE, "scs_multi_system_eval needs a multi-output context (scs_set_outputs)");
    if (!c->loss_set) fail(c, SCS_ERR_STATE, "no loss: call scs_set_loss first");
    if (!x || (G && ldg < c->m)) fail(c, SCS_ERR_ARG, "scs_multi_system_eval: null x or ldg < nvar");
    HCK(hipSetDevice(c->dev));
    const int64_t m = c->m;
    invalidate_caches(c);
    h2d(c, c->x, x, m);
    const double fv = forward(c, x, c->x, EPI_GGN);
    gemv_t_local(c, c->gN, c->gtmp);
    multi_system(c);
    if (G)
      HCK(hipMemcpy2DAsync(G, sizeof(double) * ldg, c->G, sizeof(double) * c->mpad, sizeof(double) * m, m,
                           hipMemcpyDeviceToHost, c->st));
    if (g) d2h(c, g, c->gtmp, m);
    sync(c);
    if (f) *f = fv;
    invalidate_caches(c);
    if (c->timing) tresolve(c);
  });
}

// the sample-space system of a multi-output ProxGGNSCORE step at x (the step's own forward pass and
// assembly, before the solve): M of order n1 = N·nout + 1 and b
int scs_multi_sample_system_eval(scs_ctx* c, const double* x, double* M, int64_t ldm, double* b) {
  return guarded(c, [&] {
    if (!c->has_data || c->generic) fail(c, SCS_ERR_STATE, "no data");
    if (!multi(c))
      fail(c, SCS_ERR_STATE, "scs_multi_sample_system_eval needs a multi-output context (scs_set_outputs)");
    if (!c->multi_sample)
      fail(c, SCS_ERR_STATE, "scs_multi_sample_system_eval needs the sample-space switch (multi_sample=True / "
                             "scs_set_multi_sample)");
    if (!c->loss_set) fail(c, SCS_ERR_STATE, "no loss: call scs_set_loss first");
    if (!c->reg_set || !c->smooth_set)
      fail(c, SCS_ERR_STATE, "scs_multi_sample_system_eval needs the regularizer and the smoother (h = 1 ./ Hr, λ gr)");
    if (c->ggn == SCS_GGN_NONE) fail(c, SCS_ERR_ARG, "scs_multi_sample_system_eval needs an out_fn / GGN loss kind");
    const int64_t n1 = c->Nglob * c->nout + 1;
    if (!multi_sample_shape(c))
      fail(c, SCS_ERR_ARG, "scs_multi_sample_system_eval: N*nout + 1 = %lld > d*nout = %lld is the feature branch's "
                           "shape (scs_multi_system_eval serves it)", (long long)n1, (long long)c->m);
    if (c->sparse)
      fail(c, SCS_ERR_ARG, "scs_multi_sample_system_eval: the sample-space branch of multi_sample needs a dense A");
    if (!x || (M && ldm < n1)) fail(c, SCS_ERR_ARG, "scs_multi_sample_system_eval: null x or ldm < N*nout + 1");
    HCK(hipSetDevice(c->dev));
    invalidate_caches(c);
    h2d(c, c->x, x, c->m);
    HCK(launch_smoother(c->smooth, c->x, c->m, c->mu, c->slb, c->sub, c->wel, c->gr, c->Hr, c->st));
    multi_sample_system(c, x, true);
    const SampleSys& S = c->ss;
    // Ms is row-major: its transpose lands column-major on the host through a column-major staging copy
    if (M) {
      double* T = dalloc<double>(c, (size_t)S.n1pad * S.n1pad, false);
      struct Free {
        scs_ctx* c;
        double** p;
        ~Free() {
          (void)hipStreamSynchronize(c->st);
          dfree_t(c, *p);
        }
      } fr{c, &T};
      HCK(qr_from_rowmajor(S.Ms, S.n1pad, T, S.n1pad, n1, S.n1pad, c->st));
      HCK(hipMemcpy2DAsync(M, sizeof(double) * ldm, T, sizeof(double) * S.n1pad, sizeof(double) * n1, n1,
                           hipMemcpyDeviceToHost, c->st));
      sync(c);
    }
    if (b) d2h(c, b, S.bS, n1);
    sync(c);
    invalidate_caches(c);
    if (c->timing) tresolve(c);
  });
}

int scs_timing_enable(scs_ctx* c, int on) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_timing_enable(s_, on); });
  return guarded(c, [&] {
    c->timing = on != 0;
    c->timing_every = on > 1 ? on : 1;
  });
}

int scs_timing_get(scs_ctx* c, scs_timing* t) {
  if (is_group(c)) return scs_timing_get(c->subs[0], t);   // device 0's accumulators
  return guarded(c, [&] {
    tresolve(c);
    t->gram_ms = c->tms[T_GRAM];
    t->gram_calls = c->tcalls[T_GRAM];
    t->gemv_ms = c->tms[T_GEMV];
    t->gemv_calls = c->tcalls[T_GEMV];
    t->solve_ms = c->tms[T_SOLVE];
    t->solve_calls = c->tcalls[T_SOLVE];
    t->step_ms = c->tms[T_STEP];
    t->step_calls = c->tcalls[T_STEP];
    t->reduce_ms = c->tms[T_REDUCE];
    t->reduce_calls = c->tcalls[T_REDUCE];
  });
}

int scs_kernel_names(scs_ctx* c, char* gram, int64_t gram_cap, char* product, int64_t product_cap) {
  if (is_group(c)) return scs_kernel_names(c->subs[0], gram, gram_cap, product, product_cap);
  return guarded(c, [&] {
    auto put = [](char* dst, int64_t cap, const std::string& v) {
      if (!dst || cap <= 0) return;
      const size_t n = std::min<size_t>(v.size(), (size_t)cap - 1);
      std::memcpy(dst, v.data(), n);
      dst[n] = 0;
    };
    put(gram, gram_cap, c->gram_kname);
    put(product, product_cap, c->prod_kname);
  });
}

int scs_timing_reset(scs_ctx* c) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_timing_reset(s_); });
  return guarded(c, [&] {
    tresolve(c);
    for (int i = 0; i < T_N; ++i) {
      c->tms[i] = 0;
      c->tcalls[i] = 0;
    }
  });
}

int scs_fallback_counts(scs_ctx* c, int64_t* counts, int n) {
  if (!c) return SCS_ERR_ARG;
  if (!counts || n < 0) {
    c->err = "scs_fallback_counts: bad arguments";
    return SCS_ERR_ARG;
  }
  for (int i = 0; i < n; ++i) counts[i] = 0;
  // a multi-device context: the sum over its devices
  std::vector<scs_ctx*> cs = is_group(c) ? c->subs : std::vector<scs_ctx*>{c};
  for (scs_ctx* s_ : cs)
    for (int i = 0; i < n && i < SCS_FB_N; ++i) counts[i] += s_->fb[i];
  return SCS_OK;
}

int scs_sync(scs_ctx* c) {
  if (is_group(c)) return group_run(c, [&](scs_ctx* s_, int) { return scs_sync(s_); });
  return guarded(c, [&] { sync(c); });
}

}  // extern "C"

// ===========================================================================
// Multi-device contexts (scs_create_multi): one process drives several GPUs
// ===========================================================================
// The reference's iterate! is one process (iterate.jl:56-76; no MPI / Distributed), so a Julia
// caller gets the node's GPUs from one DeviceProblem(...; devices): the library splits the rows
// (row_plan, the same blocks as one process per GPU), gives every device a sub-context with its
// rows and an RCCL communicator from ncclCommInitAll, and runs each supported call on all
// sub-contexts at once -- one host thread per device, since the step's exchange is a collective
// every device must enter.  Every sub-context computes the same replicated m-vectors with the same
// bits, so outputs are device 0's.

// One persistent host thread per device of a group (started by scs_create_multi, joined by
// group_destroy).  A call posts one job per device and waits for all of them.
struct scs_ctx::Workers {
  struct Slot {
    std::thread th;
    std::function<void()> job;
    bool has_job = false;
  };
  std::mutex mu;
  std::condition_variable cv_job, cv_done;
  std::vector<Slot> slots;
  int pending = 0;
  bool quit = false;

  explicit Workers(const std::vector<int>& devs) : slots(devs.size()) {
    for (size_t i = 0; i < devs.size(); ++i)
      slots[i].th = std::thread([this, i, d = devs[i]] {
        (void)hipSetDevice(d);   // once: the thread drives this device for the group's lifetime
        for (;;) {
          std::function<void()> job;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv_job.wait(lk, [&] { return quit || slots[i].has_job; });
            if (!slots[i].has_job) return;   // quit
            job = std::move(slots[i].job);
            slots[i].has_job = false;
          }
          job();
          {
            std::lock_guard<std::mutex> lk(mu);
            --pending;
          }
          cv_done.notify_all();
        }
      });
  }
  // run jobs[i] on worker i, all at once; returns when every job has returned
  void run(std::vector<std::function<void()>>& jobs) {
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < slots.size(); ++i) {
        slots[i].job = std::move(jobs[i]);
        slots[i].has_job = true;
      }
      pending = (int)slots.size();
    }
    cv_job.notify_all();
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
  }
  ~Workers() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    cv_job.notify_all();
    for (auto& sl : slots)
      if (sl.th.joinable()) sl.th.join();
  }
};

// The exchange of a SCS_MULTI_HOST_EXCHANGE group (scs_create_multi_ex): every device's payload goes to
// a host slot, a barrier, every device sums the slots in device order (the same bits on every device),
// writes the sum back, a second barrier (no slot is rewritten before every device has read it).  It
// needs no RCCL and no distinct devices -- several sub-contexts may share one GPU -- so the group's
// fan-out, row split and exchange run on a one-GPU box; the cost is two host copies per exchange.
// abort() releases every waiter (group_run, after a device failed).
struct scs_ctx::HostExchange {
  struct Rank {
    HostExchange* ex = nullptr;
    int rank = 0;
    std::vector<double> sum;
  };
  int n = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t gen = 0;
  bool aborted = false;
  std::vector<std::vector<double>> slot;
  std::vector<Rank> ranks;
  explicit HostExchange(int n_) : n(n_), slot((size_t)n_), ranks((size_t)n_) {
    for (int i = 0; i < n_; ++i) ranks[(size_t)i] = Rank{this, i, {}};
  }
  bool wait() {   // false once aborted, or when the others have not all arrived within 600 s
    std::unique_lock<std::mutex> lk(mu);
    if (aborted) return false;
    const uint64_t g = gen;
    if (++arrived == n) {
      arrived = 0;
      ++gen;
      cv.notify_all();
      return true;
    }
    if (!cv.wait_for(lk, std::chrono::seconds(600), [&] { return gen != g || aborted; })) {
      aborted = true;   // a device that never arrives (diverged control flow): release everyone
      cv.notify_all();
      return false;
    }
    return gen != g;
  }
  void abort() {
    std::lock_guard<std::mutex> lk(mu);
    aborted = true;
    cv.notify_all();
  }
  static int allreduce(void* dev_buf, int64_t count, void* stream, void* user) {
    Rank* rk = static_cast<Rank*>(user);
    HostExchange* ex = rk->ex;
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::vector<double>& mine = ex->slot[(size_t)rk->rank];
    mine.resize((size_t)count);
    if (hipMemcpyAsync(mine.data(), dev_buf, sizeof(double) * count, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return 2;
    if (!ex->wait()) return 1;
    rk->sum.assign(ex->slot[0].begin(), ex->slot[0].begin() + count);
    for (int r = 1; r < ex->n; ++r) {
      const double* o = ex->slot[(size_t)r].data();
      for (int64_t e = 0; e < count; ++e) rk->sum[(size_t)e] += o[e];
    }
    if (hipMemcpyAsync(dev_buf, rk->sum.data(), sizeof(double) * count, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return 2;
    return ex->wait() ? 0 : 1;
  }
};

scs_ctx::~scs_ctx() = default;

namespace {

// run f(sub, i) on every sub-context, each on its device's worker thread; the first failing
// device's code and message become the group's.  A device that fails while the others may be
// waiting inside a collective aborts the communicators after a grace period (ncclCommAbort unblocks
// them), so the call returns instead of hanging.  The abort only sets the shared flag and calls
// ncclCommAbort: the sub-contexts' rccl handles are cleared after every worker has returned (no
// other thread reads them then), and the flag stops any further RCCL call in the meantime.  The
// group is then unusable (SCS_ERR_COMM) and must be destroyed.  Unverified on hardware beyond one
// device (no multi-GPU box here): DESIGN.md §6.
template <class F>
int group_run(scs_ctx* g, F&& f) {
  if (g->group_broken) {
    g->err = "multi-device context: an earlier call aborted its communicators; destroy it";
    return SCS_ERR_COMM;
  }
  const int n = (int)g->subs.size();
  std::vector<int> rc(n, SCS_OK);
  std::atomic<int> done{0};
  std::atomic<bool> aborted{false};
  std::vector<std::function<void()>> jobs((size_t)n);
  for (int i = 0; i < n; ++i)
    jobs[(size_t)i] = [&, i] {
      scs_ctx* s = g->subs[i];
      rc[i] = f(s, i);
      done.fetch_add(1);
      if (rc[i] == SCS_OK || n == 1) return;
      for (int t = 0; t < 500 && done.load() < n; ++t) std::this_thread::sleep_for(std::chrono::milliseconds(10));
      if (done.load() < n && !aborted.exchange(true)) {
        g->comm_abort->store(true, std::memory_order_release);
        if (g->hx) g->hx->abort();
        for (scs_ctx* o : g->subs)
          if (o->rccl) (void)ncclCommAbort(o->rccl);
      }
    };
  g->workers->run(jobs);
  if (aborted.load()) {
    g->group_broken = true;
    for (scs_ctx* o : g->subs) o->rccl = nullptr;   // aborted (freed) by ncclCommAbort
  }
  for (int i = 0; i < n; ++i)
    if (rc[i] != SCS_OK) {
      g->err = "device " + std::to_string(g->subs[i]->dev) + ": " + g->subs[i]->err;
      return rc[i];
    }
  g->err.clear();
  return SCS_OK;
}

bool is_group(const scs_ctx* c) { return c && !c->subs.empty(); }

}  // namespace

extern "C" {

int scs_create_multi(const int* devs, int ndev, scs_ctx** out) { return scs_create_multi_ex(devs, ndev, 0, out); }

int scs_create_multi_ex(const int* devs, int ndev, int flags, scs_ctx** out) {
  if (!out || !devs || ndev < 1 || (flags & ~SCS_MULTI_HOST_EXCHANGE)) return SCS_ERR_ARG;
  *out = nullptr;
  const bool host = (flags & SCS_MULTI_HOST_EXCHANGE) != 0;
  scs_ctx* g = new scs_ctx();
  for (int i = 0; i < ndev && !host; ++i)
    for (int j = 0; j < i; ++j)
      if (devs[i] == devs[j]) {
        delete g;
        return SCS_ERR_ARG;   // RCCL takes one rank per GPU
      }
  for (int i = 0; i < ndev; ++i) {
    scs_ctx* s = nullptr;
    const int rc = scs_create(devs[i], nullptr, &s);
    if (rc != SCS_OK) {
      for (scs_ctx* o : g->subs) scs_destroy(o);
      delete g;
      return rc;
    }
    g->subs.push_back(s);
  }
  g->comm_abort = std::make_shared<std::atomic<bool>>(false);
  if (host) {
    g->hx.reset(new scs_ctx::HostExchange(ndev));
    for (int i = 0; i < ndev; ++i) {
      scs_ctx* s = g->subs[i];
      s->rank = i;
      s->nranks = ndev;
      s->ar = &scs_ctx::HostExchange::allreduce;
      s->ar_user = &g->hx->ranks[(size_t)i];
      s->comm_abort = g->comm_abort;
    }
  } else {
    std::vector<ncclComm_t> comms((size_t)ndev, nullptr);
    const ncclResult_t r = ncclCommInitAll(comms.data(), ndev, devs);
    if (r != ncclSuccess) {
      for (scs_ctx* o : g->subs) scs_destroy(o);
      delete g;
      return SCS_ERR_COMM;
    }
    for (int i = 0; i < ndev; ++i) {
      g->subs[i]->rccl = comms[(size_t)i];
      g->subs[i]->rank = i;
      g->subs[i]->nranks = ndev;
      g->subs[i]->comm_abort = g->comm_abort;
    }
  }
  g->workers.reset(new scs_ctx::Workers(std::vector<int>(devs, devs + ndev)));
  g->dev = devs[0];
  g->st = g->subs[0]->st;
  *out = g;
  return SCS_OK;
}

int scs_group_size(scs_ctx* c, int* ndev) {
  if (!c || !ndev) return SCS_ERR_ARG;
  *ndev = is_group(c) ? (int)c->subs.size() : 1;
  return SCS_OK;
}

int scs_comm_info(scs_ctx* c, int* kind, int* nranks, int* rank, int* rccl_version, char* lib, int64_t cap) {
  if (!c) return SCS_ERR_ARG;
  int k = SCS_COMM_NONE, n = 1, r = 0;
  const scs_ctx* s = is_group(c) ? c->subs[0] : c;
  if (is_group(c)) {
    k = c->hx ? SCS_COMM_GROUP_HOST : SCS_COMM_GROUP_RCCL;
    n = (int)c->subs.size();
    if (!c->hx && s->rccl) {   // the communicator's own view (ncclCommInitAll over the devices)
      int cn = 0;
      if (ncclCommCount(s->rccl, &cn) == ncclSuccess) n = cn;
    }
  } else if (s->rccl) {
    k = SCS_COMM_RCCL;
    int cn = 0, cr = 0;
    if (ncclCommCount(s->rccl, &cn) != ncclSuccess || ncclCommUserRank(s->rccl, &cr) != ncclSuccess) {
      c->err = "ncclCommCount / ncclCommUserRank failed";
      return SCS_ERR_COMM;
    }
    n = cn;
    r = cr;
  } else if (s->ar) {
    k = SCS_COMM_CALLBACK;
    n = s->nranks;
    r = s->rank;
  }
  if (kind) *kind = k;
  if (nranks) *nranks = n;
  if (rank) *rank = r;
  if (rccl_version) {
    int v = 0;
    *rccl_version = ncclGetVersion(&v) == ncclSuccess ? v : 0;
  }
  if (lib && cap > 0) {
    Dl_info di{};
    const char* path = (dladdr((void*)&ncclAllReduce, &di) && di.dli_fname) ? di.dli_fname : "";
    char real[4096];
    if (*path && realpath(path, real)) path = real;
    std::snprintf(lib, (size_t)cap, "%s", path);
  }
  return SCS_OK;
}

}  // extern "C"

namespace {

int group_destroy(scs_ctx* g) {
  g->workers.reset();   // joins the device threads
  for (scs_ctx* s : g->subs) scs_destroy(s);
  g->subs.clear();
  delete g;
  return SCS_OK;
}

int group_set_data(scs_ctx* g, int64_t N, int64_t m, const void* A, int in32, int64_t lda, const double* y,
                   int64_t Nglob, int64_t row0) {
  const int n = (int)g->subs.size();
  const size_t es = in32 ? sizeof(float) : sizeof(double);
  if ((Nglob > 0 && Nglob != N) || row0 != 0) {
    g->err = "a multi-device context holds the whole problem: N_global = N, row0 = 0 (it splits the rows itself)";
    return SCS_ERR_ARG;
  }
  if (A && N < n) {
    g->err = "a multi-device context needs at least one row per device";
    return SCS_ERR_ARG;
  }
  g->plan = A ? row_plan(N, n) : std::vector<RowBlock>((size_t)n);
  const int rc = group_run(g, [&](scs_ctx* s, int i) {
    const RowBlock b = g->plan[(size_t)i];
    return set_data_any(s, A ? b.rows() : 0, m, DenseSrc{A ? (const char*)A + es * b.r0 : nullptr, in32, lda},
                        y ? y + b.r0 : nullptr, A ? N : 0, b.r0);
  });
  if (rc == SCS_OK) {
    g->grpN = A ? N : 0;
    g->grpm = m;
  }
  return rc;
}

int group_gen_data(scs_ctx* g, const scs_synth* sp) {
  const int n = (int)g->subs.size();
  if (!sp || sp->row0 != 0 || sp->N != sp->N_global || sp->N < n) {
    g->err = "a multi-device context generates the whole problem: spec N = N_global >= devices, row0 = 0";
    return SCS_ERR_ARG;
  }
  g->plan = row_plan(sp->N, n);
  const int rc = group_run(g, [&](scs_ctx* s, int i) {
    scs_synth q = *sp;
    q.row0 = g->plan[(size_t)i].r0;
    q.N = g->plan[(size_t)i].rows();
    return scs_gen_data(s, &q);
  });
  if (rc == SCS_OK) {
    g->grpN = sp->N;
    g->grpm = sp->m;
  }
  return rc;
}

int group_get_data(scs_ctx* g, int64_t r0, int64_t nr, double* A, int64_t lda_out, double* y) {
  if (r0 < 0 || nr < 0 || r0 + nr > g->grpN) {
    g->err = "scs_get_data: rows out of range";
    return SCS_ERR_ARG;
  }
  for (const RowPiece& p : window_pieces(g->plan, r0, nr)) {
    scs_ctx* s = g->subs[(size_t)p.dev];
    const int rc = scs_get_data(s, p.local0, p.n, A ? A + p.off : nullptr, lda_out, y ? y + p.off : nullptr);
    if (rc != SCS_OK) {
      g->err = s->err;
      return rc;
    }
  }
  return SCS_OK;
}

// the held-out rows split like the data's (row_plan; a device may hold none of them)
int group_set_test_data(scs_ctx* g, int64_t N, const void* A, int in32, int64_t lda, const double* y, int64_t Nglob,
                        int64_t row0) {
  const size_t es = in32 ? sizeof(float) : sizeof(double);
  if ((Nglob > 0 && Nglob != N) || row0 != 0) {
    g->err = "a multi-device context holds the whole test set: N_global = N, row0 = 0";
    return SCS_ERR_ARG;
  }
  const std::vector<RowBlock> plan = row_plan(std::max<int64_t>(N, 0), (int)g->subs.size());
  return group_run(g, [&](scs_ctx* s, int i) {
    const RowBlock b = plan[(size_t)i];
    return set_test_any(s, b.rows(), DenseSrc{A ? (const char*)A + es * b.r0 : nullptr, in32, lda},
                        y ? y + b.r0 : nullptr, N, b.r0);
  });
}

int group_gen_test_data(scs_ctx* g, const scs_synth* sp) {
  if (!sp) {
    g->err = "null synth spec";
    return SCS_ERR_ARG;
  }
  const std::vector<RowBlock> plan = row_plan(sp->N, (int)g->subs.size());
  return group_run(g, [&](scs_ctx* s, int i) {
    scs_synth q = *sp;
    q.row0 = sp->row0 + plan[(size_t)i].r0;
    q.N = plan[(size_t)i].rows();
    q.N_global = sp->N;
    return scs_gen_test_data(s, &q);
  });
}

// one scalar / one m-vector out of a collective evaluation: every device runs it, device 0's result
int group_eval(scs_ctx* g, const double* x, double* out, int64_t nout,
               int (*fn)(scs_ctx*, const double*, double*)) {
  std::vector<std::vector<double>> o(g->subs.size(), std::vector<double>((size_t)std::max<int64_t>(nout, 1)));
  const int rc = group_run(g, [&](scs_ctx* s, int i) { return fn(s, x, o[(size_t)i].data()); });
  if (rc == SCS_OK && out) std::memcpy(out, o[0].data(), sizeof(double) * nout);
  return rc;
}

int group_step(scs_ctx* g, const double* x, const double* x_prev, int64_t iter, const double* grad_fx, double* x_new,
               double* dx, double* pri) {
  const size_t n = g->subs.size(), m = (size_t)g->grpm;
  std::vector<std::vector<double>> xn(n, std::vector<double>(m)), d(n, std::vector<double>(dx ? m : 1));
  std::vector<double> pr(n, 0.0);
  const int rc = group_run(g, [&](scs_ctx* s, int i) {
    return scs_step_grad(s, x, x_prev, iter, grad_fx, xn[(size_t)i].data(), dx ? d[(size_t)i].data() : nullptr,
                         &pr[(size_t)i]);
  });
  if (rc != SCS_OK) return rc;
  std::memcpy(x_new, xn[0].data(), sizeof(double) * m);
  if (dx) std::memcpy(dx, d[0].data(), sizeof(double) * m);
  if (pri) *pri = pr[0];
  return SCS_OK;
}

int group_iterate(scs_ctx* g, const double* x0, const double* x_star, int64_t max_epoch, double x_tol, double f_tol,
                  int rel_kind, double* x_out, const scs_history* h, int64_t* n_hist, int64_t* epochs) {
  const size_t n = g->subs.size(), m = (size_t)g->grpm;
  const size_t cap = (size_t)std::max<int64_t>(2 * max_epoch + 1, 1);
  std::vector<std::vector<double>> buf(n, std::vector<double>(7 * cap + m));
  std::vector<int64_t> nh(n, 0), ep(n, 0);
  const int rc = group_run(g, [&](scs_ctx* s, int i) {
    double* b = buf[(size_t)i].data();
    scs_history hi{b, b + cap, b + 2 * cap, b + 3 * cap, b + 4 * cap, b + 5 * cap, b + 6 * cap};
    return scs_iterate_ex(s, x0, x_star, max_epoch, x_tol, f_tol, rel_kind, b + 7 * cap, &hi, sizeof(hi),
                          &nh[(size_t)i], &ep[(size_t)i]);
  });
  if (rc != SCS_OK) return rc;
  const double* b = buf[0].data();
  const size_t k = (size_t)nh[0];
  double* dst[7] = {h ? h->obj : nullptr, h ? h->fval : nullptr, h ? h->pri_res_norm : nullptr, h ? h->rel : nullptr,
                    h ? h->objrel : nullptr, h ? h->times : nullptr, h ? h->fvaltest : nullptr};
  int has_test = 0;
  (void)scs_has_test(g->subs[0], &has_test);
  for (int a = 0; a < 7; ++a)
    if (dst[a] && (a < 6 || has_test)) std::memcpy(dst[a], b + a * cap, sizeof(double) * k);
  if (x_out) std::memcpy(x_out, b + 7 * cap, sizeof(double) * m);
  if (n_hist) *n_hist = nh[0];
  if (epochs) *epochs = ep[0];
  return SCS_OK;
}

}  // namespace

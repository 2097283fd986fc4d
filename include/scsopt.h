/*
 * scsopt.h -- C ABI of libscsopt, the MI355X (gfx950) implementation of the
 * SCORE inner iteration of SelfConcordantSmoothOptimization.jl.
 *
 * The reference has no FFI: its plugin boundary is Julia multiple dispatch on
 * `step!(method, model, reg_name, hμ, As, x, x_prev, ys, Cmat, iter)`
 * (src/algorithms/iterate.jl:52-54) plus the objective closures evaluated by
 * `optim_loop!` (iterate.jl:168, :189-190).  Each entry point below replaces
 * one of those Julia-side pieces; the Julia `ccall` binding a maintainer adds
 * is in INTEGRATION.md, the Python ctypes binding is
 * selfconcordantsmoothoptimization.jl_amd/scsopt/_lib.py.
 *
 * Conventions
 *   - All functions return SCS_OK (0) or an error code; the message is
 *     available from scs_last_error(ctx) (errors the reference raises with
 *     Base.error carry the reference's message text).
 *   - Host pointers are borrowed for the duration of the call.  Vectors of
 *     length m (x, x_prev, x_new, dx) are host fp64 arrays.
 *   - A is column-major (Julia Matrix{Float64} layout) with leading dimension
 *     lda >= N.  In a multi-rank context each rank holds rows
 *     [row0, row0 + N) of the global N_global x m matrix (row-sharded).
 *   - A context is not thread-safe; all device work is ordered on its stream.
 */
#ifndef SCSOPT_H
#define SCSOPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCS_OK 0
#define SCS_ERR_ARG 1      /* invalid argument / unsupported combination     */
#define SCS_ERR_HIP 2      /* HIP runtime / device failure                   */
#define SCS_ERR_SOLVE 3    /* factorization failed (singular system)         */
#define SCS_ERR_STATE 4    /* call order (e.g. step before data)             */
#define SCS_ERR_REF 5      /* an error the reference itself raises           */
#define SCS_ERR_COMM 6     /* all-reduce callback failed                     */
#define SCS_ERR_CALLBACK 7 /* a user loss callback returned non-zero         */

/* f(A, y, x) kinds -- closed forms of the reference's user callbacks.       */
enum scs_loss_kind {
  SCS_LOSS_LOGISTIC_MARGIN = 1, /* c*sum(log(1+exp(-y.*(A*x))))  test/test_algs.jl:9  */
  SCS_LOSS_LOGISTIC_CE = 2,     /* f(y, sigmoid(A*x)), cross-entropy  SURVEY §8a C3 */
  SCS_LOSS_LEAST_SQUARES = 3,   /* 0.5*sum((A*x-y).^2)*c           README.md:212-214 */
  SCS_LOSS_QUADRATIC = 4,       /* 1/2*(x'*(A*x)) + y'*x             test/test_algs.jl:90 */
  SCS_LOSS_ROSENBROCK = 5,      /* chained Rosenbrock, no data        README.md:49 */
  SCS_LOSS_CALLBACK = 6,        /* the caller's f / grad_fx / hess_fx (scs_set_loss_callback) */
  SCS_LOSS_SAMPLEWISE = 7,      /* f = sum_i l(y_i, a_i'x): the caller's l, dl/dz, d2l/dz2 on z = A*x
                                   (scs_set_loss_samplewise); the device keeps A and every product */
  /* K = nout outputs (scs_set_outputs): x = vec(X), X d x K; Y N x K; Z = A*X, P = row softmax of Z */
  SCS_LOSS_SOFTMAX_CE = 8,      /* -c*sum(Y .* log.(P)): multinomial logistic regression (Y need not be one-hot) */
  SCS_LOSS_MULTI_LS = 9         /* 0.5*c*sum((A*X .- Y).^2): multi-target least squares */
};

/* (out_fn, f(y, ŷ)) pairs used by ProxGGNSCORE (prox-GGN-SCORE.jl:44-56).    */
enum scs_ggn_kind {
  SCS_GGN_NONE = 0,
  SCS_GGN_SIGMOID_CE = 1,       /* Mfunc = sigmoid(A*x), CE on ŷ   test/test_algs.jl:10-11 */
  SCS_GGN_LINEAR_LS = 2,        /* out_fn = A*x, 0.5*c*sum((ŷ-y).^2) README.md:233-239 */
  SCS_GGN_SAMPLEWISE = 3,       /* ŷ_i = φ(a_i'x), f = sum_i l(y_i, ŷ_i): the caller's dŷ/dz, df/dŷ, d2f/dŷ2
                                   (scs_set_loss_samplewise with has_ggn) */
  SCS_GGN_LINEAR_SOFTMAX_CE = 4, /* out_fn = A*X (the logits), f(Y, ŷ) = -c*sum(Y .* log.(softmax(ŷ))): J = I_K ⊗ A */
  SCS_GGN_LINEAR_MULTI_LS = 5   /* out_fn = A*X, 0.5*c*sum((ŷ .- Y).^2) */
};

/* reg_name strings of get_reg / invoke_prox (regularizers.jl:4-31,
 * prox-operators.jl:68-79).                                                 */
enum scs_reg_kind { SCS_REG_L1 = 1, SCS_REG_L2 = 2, SCS_REG_INDBOX = 3, SCS_REG_GL = 4 };

/* Smoother types (src/regularizers/: the *-smooth.jl files).                 */
enum scs_smoother_kind {
  SCS_SMOOTH_PHUBER_L1L2 = 1,   /* PHuberSmootherL1L2(μ)          phuber-smooth.jl:27   */
  SCS_SMOOTH_PHUBER_INDBOX = 2, /* PHuberSmootherIndBox(lb,ub,μ)  phuber-smooth.jl:59   */
  SCS_SMOOTH_PHUBER_GL = 3,     /* PHuberSmootherGL(μ, problem)   phuber-smooth.jl:137  */
  SCS_SMOOTH_EXP_INDBOX = 4,    /* ExponentialSmootherIndBox      exponential-smooth.jl:28 */
  SCS_SMOOTH_LOGEXP_INDBOX = 5, /* LogExpSmootherIndBox(lb,ub,μ)  log-exp-smooth.jl:28 */
  SCS_SMOOTH_OSBA_L1L2 = 6,     /* OsBaSmootherL1L2(μ)            ostrovskii-bach-smooth.jl:27 */
  SCS_SMOOTH_OSBA_GL = 7        /* OsBaSmootherGL(μ, problem)     ostrovskii-bach-smooth.jl:59 */
};

/* ProximalMethod subtypes (src/algorithms/prox-*-SCORE.jl).                 */
enum scs_method_kind { SCS_PROX_NSCORE = 1, SCS_PROX_GGNSCORE = 2, SCS_PROX_LQNSCORE = 3 };

typedef struct scs_ctx scs_ctx;

/* All-reduce hook for row-sharded contexts: sum `count` fp64 values in place
 * across ranks.  `dev_buf` is the device buffer registered with
 * scs_set_reduce_buffer (offset 0); `stream` is the context stream.  Return 0
 * on success.  Called between the local partial Gram/gradient and the m x m
 * solve (the only exchange point of the path).              */
typedef int (*scs_allreduce_fn)(void* dev_buf, int64_t count, void* stream, void* user);

/* Synthetic on-device data (counter-based RNG; every row is reproducible from
 * its global index, so any row shard is generated in place).               */
typedef struct scs_synth {
  int64_t N_global;  /* total rows                                        */
  int64_t row0;      /* first global row held by this context             */
  int64_t N;         /* rows held by this context                         */
  int64_t m;         /* columns                                           */
  uint64_t seed;
  int kind;          /* 1: A ~ N(0,1)/sqrt(m); y ~ Bernoulli(sigmoid(A x_true)) in {0,1}
                        2: A ~ N(0,1)/sqrt(m); y ~ ±1 with P(+1) = sigmoid(A x_true)
                        3: A ~ N(0,1);         y = A x_true + 0.1 eps
                        4: sparse A (scs_gen_sparse); x_true ~ U(-1.5,1.5), y = A x_true + 0.1 eps */
  double density;    /* fraction of nonzero entries of x_true             */
} scs_synth;

/* Per-kernel device-time accumulators (hipEvent elapsed, ms), read by bench. */
typedef struct scs_timing {
  double gram_ms;    int64_t gram_calls;   /* MFMA Aᵀ diag(w) A                */
  double gemv_ms;    int64_t gemv_calls;   /* A*x and Aᵀ*v streaming passes    */
  double solve_ms;   int64_t solve_calls;  /* m x m factor + solve             */
  double step_ms;    int64_t step_calls;   /* whole scs_step                   */
  double reduce_ms;  int64_t reduce_calls; /* all-reduce callback              */
} scs_timing;

/* ---- lifecycle ---------------------------------------------------------- */
const char* scs_version(void);
/* Create a context on HIP device `device`; `stream` = existing hipStream_t or
 * NULL to create one.                                                       */
int scs_create(int device, void* stream, scs_ctx** out);
int scs_destroy(scs_ctx* ctx);
/* One process, several GPUs (the reference's iterate! is one process, iterate.jl:56-76): a context
 * over devs[0..ndev) that splits the problem's rows across them (contiguous balanced blocks, the
 * first N % ndev devices one more row -- the blocks of one process per GPU), with an RCCL
 * communicator over the devices (ncclCommInitAll; one GPU each).  scs_set_data / scs_gen_data
 * take the WHOLE problem (N_global = N, row0 = 0); the problem / method / step / loop entry
 * points (scs_set_loss ... scs_iterate, scs_eval_*, scs_step*, scs_set_batches, timing) run on
 * every device at once, one host thread each, and return device 0's results (every device
 * holds the same replicated x and m-vectors).  scs_get_data gathers rows across devices;
 * kernel-level entry points and sparse data take a single-device context (SCS_ERR_ARG).
 * ndev = 1 is a plain one-device run.  A device that fails inside a collective aborts the
 * communicators (then every call returns SCS_ERR_COMM: destroy the context).                 */
int scs_create_multi(const int* devs, int ndev, scs_ctx** out);
/* The same with flags.  SCS_MULTI_HOST_EXCHANGE: the group's exchange through host memory instead of
 * RCCL (every device's payload to a host slot, a barrier, the slots summed in device order on every
 * device, written back) -- no RCCL, and devs may repeat a GPU (several sub-contexts on one device:
 * the group's fan-out, row split and exchange on a one-GPU machine).  Two host copies per exchange.  */
#define SCS_MULTI_HOST_EXCHANGE 1
int scs_create_multi_ex(const int* devs, int ndev, int flags, scs_ctx** out);
/* Devices of a context (1 for scs_create).                                                   */
int scs_group_size(scs_ctx* ctx, int* ndev);
const char* scs_last_error(const scs_ctx* ctx);
int scs_get_stream(scs_ctx* ctx, void** stream);

/* ---- row sharding ------------------------------------------------------- */
/* Two ways to run the exchange step (one in-place fp64 sum per step):
 *  (a) libscsopt's own RCCL communicator (the default of the Python and Julia hosts on GPUs):
 *      rank 0 calls scs_rccl_unique_id, the caller hands the 128 opaque bytes to every rank
 *      (MPI, torch.distributed, a file ...), and every rank calls scs_set_comm_rccl -- a
 *      collective call.  The context then calls ncclAllReduce itself, on its stream, in place
 *      in its reduce buffer (allocated by the library unless one is registered);
 *  (b) an all-reduce callback (scs_set_comm), e.g. torch.distributed with gloo for CPU tests. */
int scs_set_comm(scs_ctx* ctx, int rank, int nranks, scs_allreduce_fn fn, void* user);
int scs_rccl_unique_id(void* id /* 128 bytes */);
int scs_set_comm_rccl(scs_ctx* ctx, int rank, int nranks, const void* id /* 128 bytes */);
/* Run the exchange path (packed Gram tiles -> all-reduce -> unpack) even at one rank, so the
 * communicator is exercised on a one-GPU host (results are unchanged).                        */
int scs_set_comm_force(scs_ctx* ctx, int on);
/* Device buffer (>= scs_reduce_buffer_size() doubles) owned by the caller,
 * used as the in-place all-reduce payload.  The size depends on the data and
 * on the registered batch list (the sample-space all-gather of batches with
 * N_global + 1 <= m): query it again after scs_set_batches.                 */
int scs_reduce_buffer_size(scs_ctx* ctx, int64_t* ndoubles);
/* What the exchange actually runs on, read back from the library (for run records / scaling
 * checks): *kind = SCS_COMM_NONE / _RCCL (scs_set_comm_rccl) / _CALLBACK (scs_set_comm) /
 * _GROUP_RCCL (scs_create_multi) / _GROUP_HOST (SCS_MULTI_HOST_EXCHANGE); *nranks / *rank from the
 * communicator itself (ncclCommCount / ncclCommUserRank for RCCL; the group's device count and 0
 * for a group; the caller's values for a callback); *rccl_version = ncclGetVersion; lib (cap
 * bytes, may be NULL) = the path of the RCCL shared object this process resolved ncclAllReduce
 * from (dladdr).  Any output pointer may be NULL.                                              */
#define SCS_COMM_NONE 0
#define SCS_COMM_RCCL 1
#define SCS_COMM_CALLBACK 2
#define SCS_COMM_GROUP_RCCL 3
#define SCS_COMM_GROUP_HOST 4
int scs_comm_info(scs_ctx* ctx, int* kind, int* nranks, int* rank, int* rccl_version, char* lib, int64_t cap);
int scs_set_reduce_buffer(scs_ctx* ctx, void* dev_ptr, int64_t ndoubles);

/* ---- user callbacks (Problem(x0, f, λ; grad_fx, hess_fx), problems.jl:44-59; call sites
 * prox-N-SCORE.jl:49-56, prox-L-BFGS-SCORE.jl:85-91, iterate.jl:168) -------------------
 * SCS_LOSS_CALLBACK evaluates the loss on the caller's side (a data problem's closure captures
 * its own A, y: the device holds no data, as for a ProblemGeneric -- scs_set_data(N = 0,
 * A = NULL, m)); the smoother, the m x m solve, damping, prox and the loop stay on the device.
 * `what`: SCS_CB_F    out[0] = f(x)
 *         SCS_CB_GRAD out[0..m) = grad_fx(x)
 *         SCS_CB_HESS out = hess_fx(x), m x m column-major (ProxNSCORE)
 *         SCS_CB_FTEST out[0] = f(Atest, ytest, x), the held-out loss (iterate.jl:173), asked
 *                     only after scs_set_test_callback(ctx, 1)
 *         SCS_CB_GGN  out = [J (n x m, column-major) | r (n) | q (n)] with n = ggn_rows:
 *                     J = jac_yx, r = grad_fy, Q = diag(q) = hess_fy (prox-GGN-SCORE.jl:44-49);
 *                     a general symmetric Q is passed eigen-rotated (J̃ = VᵀJ, r̃ = Vᵀr,
 *                     q = its eigenvalues), which leaves JᵀQJ, Jᵀr and the sample-space
 *                     system of ggn_score_step unchanged (ProxGGNSCORE; multi-output targets
 *                     ny > 1 are n = N·ny rows)
 *         SCS_CB_GRAD_X out[0..m) = grad_fx(x) called with x ALONE: ProxGGNSCORE builds
 *                     grad_f = x -> model.grad_fx(x) (prox-GGN-SCORE.jl:58-59) and its ss_type 3
 *                     line search calls it (:83-84, utils.jl:31).  A data problem's
 *                     grad_fx(A, y, x) has no one-argument method: return SCS_CB_NO_METHOD and
 *                     the calling function fails with SCS_ERR_REF "MethodError: no method
 *                     matching grad_fx(::Vector{Float64})", the reference's error
 * x (m) and out are host arrays owned by the library, valid for the call; return 0 on
 * success, SCS_CB_NO_METHOD as above, anything else fails the calling ABI function with
 * SCS_ERR_CALLBACK.  There is no automatic differentiation on this path: ProxNSCORE needs
 * SCS_CB_HESS, ProxGGNSCORE ggn_rows > 0.                                                  */
#define SCS_CB_F 0
#define SCS_CB_GRAD 1
#define SCS_CB_HESS 2
#define SCS_CB_GGN 3
#define SCS_CB_FTEST 4
#define SCS_CB_GRAD_X 5
#define SCS_CB_NO_METHOD 2
typedef int (*scs_loss_fn)(void* user, int what, const double* x, int64_t m, double* out);
int scs_set_loss_callback(scs_ctx* ctx, scs_loss_fn fn, void* user, int64_t ggn_rows);

/* ---- sample-wise losses outside the menu: f(A, y, x) = sum_i l(y_i, z_i), z = A*x ---------
 * SCS_LOSS_SAMPLEWISE keeps the data and every product with A on the device (dense fp64 / fp32,
 * sparse, both device doors, row shards, minibatches, the held-out set); the caller supplies N
 * numbers per derivative from z and y.  `what` is a bit set:
 *   SCS_SW_VALUE  val[i] = l(y_i, z_i), already scaled (the library applies no scale)
 *   SCS_SW_D1     d1[i]  = dl/dz_i
 *   SCS_SW_D2     d2[i]  = d2l/dz_i2
 *   SCS_SW_GGN    s[i] = dŷ_i/dz_i, d1[i] = r_i = df/dŷ_i, d2[i] = q_i = d2f/dŷ_i2 (a diagonal
 *                 hess_fy; prox-GGN-SCORE.jl:44-49 with ŷ_i = φ(z_i)); never together with D1 / D2
 * n: the rows of the view in use (this rank's data rows, a minibatch view, the held-out view --
 * ftest is the same callback on that view's z, y); z, y and every output have n entries; outputs
 * not asked for must not be written.  device_ptrs = 0: host arrays owned by the library (z and
 * the requested outputs cross per call, y once per view), `stream` is NULL.  device_ptrs = 1: the
 * library's device buffers and the context's stream: the callback queues its work on that stream
 * (or completes it before it returns); the library does not synchronise around the call.  Return
 * 0; anything else fails the calling function with SCS_ERR_CALLBACK.
 * scs_set_loss(ctx, SCS_LOSS_SAMPLEWISE, SCS_GGN_NONE | SCS_GGN_SAMPLEWISE, 1.0) selects it
 * (scale != 1 and SCS_GGN_SAMPLEWISE without has_ggn: SCS_ERR_ARG).  A multi-device group
 * context is refused (SCS_ERR_ARG): its devices run one host thread each.  There is no automatic
 * differentiation: ProxNSCORE asks D2, ProxGGNSCORE GGN.  scs_iterate's fused ProxLQNSCORE epoch
 * (m >= 16384) is not taken by this kind: the unfused device-resident epoch runs instead.
 * (scs_samplewise_fn is declared as a function type and passed by pointer.)                  */
#define SCS_SW_VALUE 1
#define SCS_SW_D1 2
#define SCS_SW_D2 4
#define SCS_SW_GGN 8
typedef int (scs_samplewise_fn)(void* user, int what, int64_t n, const double* z, const double* y, double* val,
                                double* d1, double* d2, double* s, void* stream);
int scs_set_loss_samplewise(scs_ctx* ctx, scs_samplewise_fn* fn, void* user, int device_ptrs, int has_ggn);

/* ---- multi-output targets (optim_loop! reads ny = size(model.y, 2), iterate.jl:106) -----------
 * scs_set_outputs(ctx, nout), 2 <= nout <= 16, is called BEFORE the data door.  After it the m of
 * scs_set_data / scs_set_data_f32 / scs_set_data_device is A's column count d; y is N x nout,
 * column-major with leading dimension N (a host pointer, or for the device door a host or device
 * one); every vector-length argument elsewhere (x0, x, x_star, bounds, groups, gradients, x_out)
 * has nvar = d*nout entries: x = vec(X), X d x nout column-major, entry (j, l) at j + d*l.  The
 * held-out doors take N x nout targets likewise.  The loss is SCS_LOSS_SOFTMAX_CE or
 * SCS_LOSS_MULTI_LS (with SCS_GGN_LINEAR_SOFTMAX_CE / SCS_GGN_LINEAR_MULTI_LS for ProxGGNSCORE):
 *   grad f = vec(Aᵀ R), R = c (s_i P_ik - Y_ik) | c (Z - Y), s_i = sum_k Y_ik;
 *   block (k, l) of JᵀQJ = hess f is Aᵀ diag(w_kl) A, w_kl,i = c s_i (δ_kl P_ik - P_ik P_il) | c δ_kl,
 * one weighted Gram of the unchanged kernel per pair k <= l (one in all for the least squares),
 * placed into the order-nvar system.  A stays on the device as one N x d block (fp64 or fp32
 * storage): the products A X and Aᵀ R read it once for all nout columns.
 * Refused with SCS_ERR_ARG: nout outside 2..16 (nout = 0 clears the mode); with nout set: a
 * sparse A (scs_set_sparse*, scs_set_test_sparse*) unless scs_set_sparse_outputs is on (below),
 * scs_gen_sparse, scs_gen_data, scs_set_compute_f32, nranks > 1 and multi-device contexts,
 * scs_set_batches unless scs_set_multi_batches is on (below: a dense A), any other loss kind, and
 * ProxGGNSCORE when N*nout + 1 <= d*nout (the reference then takes its sample-space branch, whose
 * step differs: scs_set_multi_sample below runs it on a dense A; without it use the callback
 * loss).  The mode persists across data doors, as scs_set_dense_f32 does.                        */
/* (With nout set scs_get_dims reports A's column count d as m, scs_get_data returns y as nr x nout
 * with leading dimension nr, and the single-vector kernel-level doors -- scs_gemv_n_eval,
 * scs_gemv_t_eval, scs_gram_eval, scs_solve_eval, scs_gram_atv_eval, scs_sample_gram_eval -- are
 * refused: scs_multi_products_eval / scs_multi_system_eval below serve it.)                       */
int scs_set_outputs(scs_ctx* ctx, int nout);
/* nout (1 when unset) and nvar = the length of x.  Either pointer may be NULL.                   */
int scs_get_outputs(scs_ctx* ctx, int* nout, int64_t* nvar);
/* Multi-output losses on a sparse A (opt-in; off by default).  With the mode on and nout set,
 * scs_set_sparse / scs_set_sparse_device / scs_set_test_sparse / scs_set_test_sparse_device accept a
 * sparse A of d columns (m = d at the door, y N x nout as above): the blocked copies are cut for
 * nout right-hand sides and A X, Aᵀ R read the nonzeros once for all nout columns (per (row,
 * column): entries in ascending index within each 16384-index group, groups summed in order; bitwise
 * run to run).  The order-nvar system takes the sparse A's Gram routes on the d-column view.
 * SCS_MULTI_SPARSE_KERNEL=0 (read at the data door) forms each column with the single-vector product
 * instead.  ptr of the finer blocked copies grows to (sub-blocks x rows) int64 per direction.  Called
 * before the data door; persists across doors; stored without effect while nout is unset; refused on
 * multi-device contexts as scs_set_outputs is.  Still refused with nout set: scs_set_compute_f32,
 * scs_gen_sparse / scs_gen_data, batches (scs_set_sparse_batches included), nranks > 1, the GGN
 * sample-space shape and the single-vector kernel doors; scs_set_sparse_sample is stored without
 * effect.                                                                                          */
int scs_set_sparse_outputs(scs_ctx* ctx, int on);
/* ProxGGNSCORE's sample-space branch of a multi-output loss (opt-in; off by default).  With the
 * switch on, nout = K set and N*K + 1 <= d*K, a ProxGGNSCORE step solves the reference's
 * sample-space system (prox-GGN-SCORE.jl:124-127, J = I_K (x) A) of order n1 = N*K + 1 on the device
 * instead of being refused.  Rows and columns (i, k) = i + N*k, last index n = N*K; h = 1 ./ Hr,
 * P_l = A diag(h_l) Aᵀ, u_l = A (h_l .* lambda gr_l), Q_i the K x K block of hess_fy:
 *   M[(i,k),(j,l)] = δ_ij δ_kl + Q_i[k,l] P_l[i,j],  M[(i,k),n] = sum_l Q_i[k,l] u_l[i],  M[n,:] = e_n,
 *   b = [vec(R); 1],  d_l = -h_l .* (Aᵀ B_l + lambda gr_l B[n]).
 * K Grams of the single-output sample-space launch (one N x N buffer), one assembly launch per
 * column block, the LU (the QR in SCS_SOLVER_REFERENCE mode) of the order-n1 system.  Memory: the
 * transposed copy of A (N x d doubles), N² and n1² doubles.  With N*K + 1 > d*K the feature branch
 * runs as with the switch off; ProxNSCORE / ProxLQNSCORE are unaffected; stored without effect
 * while nout is unset.  Still refused (SCS_ERR_ARG) in the sample-space shape with the switch on: a
 * sparse A (scs_set_sparse_outputs included) -- the branch needs a dense A.  Refused on multi-device
 * contexts as scs_set_outputs is.                                                                  */
int scs_set_multi_sample(scs_ctx* ctx, int on);
/* Minibatches of a multi-output loss (opt-in; off by default: scs_set_batches then refuses a context
 * with nout set).  With the switch on and nout = K set, scs_set_batches accepts a context that holds
 * a dense A (fp64 or fp32 storage, the host or the device door): scs_select_batch gathers the
 * batch's n_b rows of A (the d-column view, the source's element type) and of Y (n_b x K) into a
 * pooled view in one launch, and a step on it is the step of a context holding A[rows_b],
 * Y[rows_b].  f, get_reg, the histories and the held-out loss stay on the full data.  ProxGGNSCORE
 * picks its branch per batch: n_b*K + 1 > d*K the feature branch, otherwise the sample-space branch
 * with scs_set_multi_sample on and its refusal (raised at that batch's step, naming n_b) with it
 * off.  SCS_MULTI_GATHER=0 (read at scs_set_batches) gathers with the single-output kernel over the
 * d-column view plus one launch per further target column instead: the same bits.  A sparse A
 * (scs_set_sparse_outputs included) stays refused at scs_set_batches: a dense A is needed.  Stored
 * without effect while nout is unset; changing it drops the pooled batch views, and switching it
 * off with a list registered on a multi-output context clears the list.  Refused on multi-device
 * contexts as scs_set_outputs is.                                                                  */
int scs_set_multi_batches(scs_ctx* ctx, int on);
/* Minibatches with nout set on a sparse A (off by default).  With on != 0 -- and scs_set_multi_batches
 * on, which stays the gate -- scs_set_batches also accepts a multi-output context whose sparse A came
 * through scs_set_sparse / scs_set_sparse_device in the scs_set_sparse_outputs mode (fp64 or fp32
 * values).  By default a batch is a densified view, the reference's (Matrix(As'), Matrix(ys')): its
 * rows of the d-column CSR written into a dense n_b x d block and Y_b gathered, after which a step
 * runs the dense multi-output path (all three methods; ProxGGNSCORE picks its branch per batch as
 * under scs_set_multi_batches) and equals the step of a dense context holding A[rows_b], Y[rows_b].
 * With scs_set_sparse_batches also on, ProxLQNSCORE's batches are sparse K-column views instead: the
 * blocked copies scs_set_sparse would build from A[rows_b], Y[rows_b] in the scs_set_sparse_outputs
 * mode, kept and refilled under scs_set_sparse_batches' budget rules; scs_set_sparse_sample stays
 * without effect.  On those views the one-pass K-column kernel runs with 256 rows per workgroup
 * where that measured faster (nout > 4) and with 1024 otherwise; SCS_MULTI_SPARSE_NARROW=0 / 1 (read
 * at scs_set_batches) forces 1024 / 256: the same bits.
 * scs_multi_products_eval on a context with a selected sparse view runs on that view (V is n_b x K);
 * scs_get_batch_data returns the batch's rows densified, and Y_b; scs_batch_info counts both kinds
 * of view.  Stored without effect while nout is unset or on a dense A; changing it drops the pooled
 * batch views, and switching it off with a list registered on a sparse multi-output context clears
 * the list.  Refused on multi-device contexts as scs_set_outputs is.                              */
int scs_set_multi_sparse_batches(scs_ctx* ctx, int on);

/* ---- data  (Problem(A, y, ...) -- problems.jl:61-81) --------------------- */
/* Upload host A (column-major, N x m, leading dim lda) and y (N).  N is the
 * local row count; N_global/row0 describe the shard.  A may be NULL with
 * m > 0 for a ProblemGeneric (problems.jl:44-59): SCS_LOSS_ROSENBROCK or SCS_LOSS_CALLBACK. */
int scs_set_data(scs_ctx* ctx, int64_t N, int64_t m, const double* A, int64_t lda,
                 const double* y, int64_t N_global, int64_t row0);
int scs_gen_data(scs_ctx* ctx, const scs_synth* spec);
/* ---- fp32 storage of a dense A  (Problem(A::Matrix{Float32}, y, x0::Vector{Float64}, ...):
 * A::DataTupleOrArray2 admits any Real element type, problems.jl:61-62, types/custom.jl:15, and
 * Julia promotes every product with the Float64 x to Float64 -- fp32 values, fp64 arithmetic).
 * on = 1: the dense row blocks uploaded or generated AFTER the call (scs_set_data, scs_gen_data,
 * scs_set_test_data, scs_gen_test_data, and the minibatch views gathered from them) are stored as
 * fp32 on the device, half the memory and half the bytes of every pass over A; fp64 input is
 * rounded to nearest even while the panel-blocked block is written, and scs_gen_data forms y from
 * the stored (rounded) rows.  Every kernel widens the stored values on load and runs the fp64
 * kernel's arithmetic in its order, so an fp32-stored context produces, bit for bit, what an
 * fp64-stored context produces from the same values widened to fp64 (products, Gram, Aᵀv, x,
 * every history array).  Weights, y, z, the Gram, the factorizations and all m-vectors stay fp64;
 * scs_set_compute_f32 is independent of this.  scs_get_data / scs_get_columns return the stored
 * values widened.  The mode persists across scs_set_data (as scs_set_solver's choice does).  No
 * effect on sparse data (its dense mirror and dense batches stay fp64).  Default 0.
 * With fp32-stored data the main Gram runs the default interleaved kernel whatever SCS_GRAM_SIA /
 * SCS_GRAM_GLDS select.  SCS_LOSS_QUADRATIC (an m x m operator A) is refused with SCS_ERR_ARG.  */
int scs_set_dense_f32(scs_ctx* ctx, int on);
/* Host fp32 rows (float, column-major, N x m, leading dim lda), stored as they are: the host never
 * widens them.  Switches the mode on, as scs_set_dense_f32(ctx, 1) would.  A32 points to float
 * (void*: bindings pass an untyped pointer); it must not be NULL.                             */
int scs_set_data_f32(scs_ctx* ctx, int64_t N, int64_t m, const void* A32, int64_t lda,
                     const double* y, int64_t N_global, int64_t row0);
/* a_elem_bytes: element size of the dense A (8, or 4 when stored fp32); a_bytes: bytes of that block
 * (0 without one); ctx_bytes: device bytes the context holds now, summed over its own allocations
 * (a multi-device context: device 0's element size, bytes summed).  Any pointer may be NULL.    */
int scs_data_info(scs_ctx* ctx, int* a_elem_bytes, int64_t* a_bytes, int64_t* ctx_bytes);
/* ---- a dense A that is already on the device  (a torch-ROCm tensor, a CuPy array, a ROCArray) ---
 * dA is device memory on the context's device (checked with hipPointerGetAttributes before anything
 * is launched; anything else is refused with SCS_ERR_ARG).  Element (n, j) of the N x m matrix sits
 * at dA[n*stride_n + j*stride_m], elements of elem_bytes = 8 (double) or 4 (float).  Strides are in
 * elements and one of them must be 1: stride_m = 1 with stride_n >= m is a row-major matrix (the
 * NumPy / torch default, or a column slice of a wider one), stride_n = 1 with stride_m >= N a
 * column-major one.  One kernel pass re-tiles the matrix into the panel-blocked block on the
 * context's stream, zero padding included: no staging buffer, no host copy, no memset.  Peak device
 * memory is the source plus the tiled block.
 * The stored type is the context's mode alone (scs_set_dense_f32): unlike scs_set_data_f32 an fp32
 * source does not switch it on, and all four source x storage pairs are legal (a double source into
 * fp32 storage is rounded to nearest even, a float source into fp64 storage widened).  The stored
 * block is bit for bit what scs_set_data / scs_set_data_f32 store from the same values.
 * y (N doubles) may be a host or a device pointer; the library asks the pointer's attributes.
 * src_stream: the stream the producer of dA (and of a device y) ran on; the context's stream waits
 * for the work already queued on it (event record + wait).  NULL: the caller guarantees the source is
 * complete.  The two values of __cuda_array_interface__ are taken as well: (void*)1, the legacy default
 * stream (the event is recorded on the NULL stream), and (void*)2, the per-thread default stream (the
 * library synchronises the device instead); neither is handed to the runtime as a handle.  The call returns after the context's stream is synchronised, so the source may be freed
 * on return.  N_global / row0 describe the shard as in scs_set_data.  Refused with SCS_ERR_ARG:
 * elem_bytes other than 4 or 8, two non-unit strides, a stride smaller than the extent it spans, a
 * NULL dA, and a multi-device context (scs_create_multi*: it would have to split the device array). */
int scs_set_data_device(scs_ctx* ctx, int64_t N, int64_t m, const void* dA, int elem_bytes,
                        int64_t stride_n, int64_t stride_m, const double* y, void* src_stream,
                        int64_t N_global, int64_t row0);
/* ---- held-out data (Problem(A, y, x0, f, λ; Atest, ytest), problems.jl:27-28,67-68) -------
 * optim_loop! evaluates ftest(x) = f(Atest, ytest, x) with the problem's own f (same loss kind,
 * same scale literal) at every stats push when BOTH Atest and ytest are given (iterate.jl:169-175,
 * utils.jl:55-57); the values become Solution.fvaltest (scs_history.fvaltest).  Call after the
 * data (a new scs_set_data / scs_gen_data / scs_set_sparse drops the test set).  Row-sharded
 * contexts pass their shard of the held-out rows (N local rows of N_global, every rank calls,
 * a rank may hold none); a multi-device context takes the whole set (N_global = N, row0 = 0)
 * and splits it like the data.  A = y = NULL clears the test set; exactly one of A, y NULL is the
 * reference's xor case (only one of Atest / ytest given, iterate.jl:170-171): recorded, and
 * scs_iterate_ex then raises the reference's UndefVarError at its first stats push.             */
int scs_set_test_data(scs_ctx* ctx, int64_t N, const double* A, int64_t lda, const double* y,
                      int64_t N_global, int64_t row0);
/* The same with host fp32 rows (Atest::Matrix{Float32}), stored as they are; switches the fp32
 * storage mode on (scs_set_dense_f32).  Dense held-out rows of an fp32-mode context are fp32.   */
int scs_set_test_data_f32(scs_ctx* ctx, int64_t N, const void* A32, int64_t lda, const double* y,
                          int64_t N_global, int64_t row0);
/* The same from a device matrix (N x the data's m), as scs_set_data_device takes it; dA and y are
 * both required.                                                                               */
int scs_set_test_data_device(scs_ctx* ctx, int64_t N, const void* dA, int elem_bytes,
                             int64_t stride_n, int64_t stride_m, const double* y, void* src_stream,
                             int64_t N_global, int64_t row0);
/* CSR held-out rows (0-based, m columns; values stored fp64, or fp32 with val_f32 = 1).       */
int scs_set_test_sparse(scs_ctx* ctx, int64_t N, int64_t nnz, const int64_t* rowptr, const int32_t* colidx,
                        const double* val, int val_f32, const double* y, int64_t N_global, int64_t row0);
/* Rows [row0, row0 + N) of the scs_gen_data generator (dense kinds 1-3, spec->m = the data's m):
 * with row0 >= the data's N_global they are held-out samples of the same distribution.  A
 * multi-device context splits spec->N rows across its devices.                                */
int scs_gen_test_data(scs_ctx* ctx, const scs_synth* spec);
/* A callback loss (SCS_LOSS_CALLBACK) keeps its held-out data on the caller's side: on = 1 makes
 * the loop ask SCS_CB_FTEST at every push.                                                     */
int scs_set_test_callback(scs_ctx* ctx, int on);
/* ftest(x) now; *on = 1 when the context holds test data.                                      */
int scs_eval_ftest(scs_ctx* ctx, const double* x, double* fval);
int scs_has_test(scs_ctx* ctx, int* on);

/* Copy device A rows [r0, r0+nr) (column-major, lda_out) and y back.       */
int scs_get_data(scs_ctx* ctx, int64_t r0, int64_t nr, double* A, int64_t lda_out, double* y);
int scs_get_dims(scs_ctx* ctx, int64_t* N, int64_t* m, int64_t* N_global, int64_t* row0);

/* ---- sparse A  (Problem(A::SparseMatrixCSC, y, ...); README.md:105 builds it
 * with sprandn(N, m, 0.01) -- BASELINE configs[4]).  Held twice on the device:
 * CSR for A*x and a CSC copy for Aᵀ*v, so both products are gathers with a
 * fixed summation order (no atomics).  Indices are 0-based; the CSC copy
 * describes the same local rows (rowidx in [0, N)).  val_f32 = 1 stores the
 * values as fp32 (the fp32-value arm of the study; accumulation stays fp64).
 * All methods run on sparse A: the products stay sparse; ProxNSCORE /
 * ProxGGNSCORE form their Gram on a dense device mirror of A, built once and
 * refused (SCS_ERR_ARG) when it does not fit in device memory.               */
int scs_set_sparse(scs_ctx* ctx, int64_t N, int64_t m, int64_t nnz,
                   const int64_t* rowptr, const int32_t* colidx, const double* val,
                   const int64_t* colptr, const int32_t* rowidx, const double* valT,
                   int val_f32, const double* y, int64_t N_global, int64_t row0);
/* Synthetic sparse A (single context): k = round(density*m) nonzeros per row
 * in a layered-bijection pattern (N a power of two, m | N; every column then
 * holds k*N/m), values N(0,1)/sqrt(k); x_true ~ U(-1.5, 1.5) and
 * y = A x_true + 0.1 eps (spec->kind must be 4; spec->density is ρ).        */
int scs_gen_sparse(scs_ctx* ctx, const scs_synth* spec, int val_f32);
int scs_get_nnz(scs_ctx* ctx, int64_t* nnz);
/* CSR copy back to the host (values widened to fp64).                       */
int scs_get_sparse(scs_ctx* ctx, int64_t* rowptr, int32_t* colidx, double* val);
/* The CSC copy back to the host, as scs_get_sparse returns the CSR one: m + 1 column pointers,
 * nnz row indices and values (widened), rows ascending within a column.                        */
int scs_get_sparse_csc(scs_ctx* ctx, int64_t* colptr, int32_t* rowidx, double* valT);
/* ---- a sparse A that is already on the device  (torch.sparse_csr_tensor, a CuPy csr_matrix, a
 * triple of ROCArrays).  A CSR is all the caller supplies: d_rowptr (N + 1 entries of ptr_bytes = 4,
 * int32, or 8, int64), d_colidx (nnz entries of idx_bytes = 4 or 8, 0-based) and d_val (nnz entries
 * of val_bytes = 4, float, or 8, double), device memory on the context's device.  All pointer x index
 * widths are legal, and val_f32 alone decides the stored type (a double source with val_f32 = 1 is
 * rounded to nearest even, a float source with val_f32 = 0 widened).  With nnz = 0, d_colidx and
 * d_val may be NULL.  One pass reads the source, validates it and writes the context's CSR; the CSC
 * copy is built on the device from the row-sorted CSR (an integer counting pass over runs of equal
 * column indices, a scan, a placing pass, and the per-column sort the host door runs too).  Column
 * indices may be unsorted within a row and (row, column) pairs may repeat: duplicates are kept, not
 * summed, in storage order.  After the call the context holds, bit for bit, what scs_set_sparse
 * holds from the same CSR arrays and their stable transposition (scipy's tocsr -> tocsc), whatever
 * the order in which the device's waves arrived.  Peak device memory is the host door's plus the
 * source; until the validation has passed, the earlier data is kept as well.
 * y and src_stream are scs_set_data_device's: y (N doubles) may be a host or a device pointer;
 * src_stream is NULL, (void*)1, (void*)2 or the producer's stream; the call returns with the
 * context's stream synchronised, so the source may be freed on return.
 * Refused with SCS_ERR_ARG, before anything of the context is freed: ptr_bytes / idx_bytes /
 * val_bytes other than 4 or 8; a NULL d_rowptr, or a NULL d_colidx / d_val with nnz > 0; a pointer
 * that hipPointerGetAttributes does not report as device memory of the context's device; an array
 * that runs past its allocation (hipMemGetAddressRange); rowptr[0] != 0, rowptr[N] != nnz or a
 * decreasing rowptr (the message names the first offending row); a column index outside [0, m),
 * compared in the source width (the message names the first offending position); nnz above
 * 2^32 - 1 (the sorts count their items in 32 unsigned bits; scs_set_sparse's INT32_MAX * 64 lies
 * above that and is refused a fortiori); a multi-device context.  The validation runs on the device and never reads outside
 * the source arrays, whatever they hold.                                                          */
int scs_set_sparse_device(scs_ctx* ctx, int64_t N, int64_t m, int64_t nnz,
                          const void* d_rowptr, int ptr_bytes, const void* d_colidx, int idx_bytes,
                          const void* d_val, int val_bytes, int val_f32, const double* y,
                          void* src_stream, int64_t N_global, int64_t row0);
/* CSR held-out rows from the device (N x the data's m), as scs_set_sparse_device takes them; the
 * arrays and y are both required.  No CSC copy is built, as for scs_set_test_sparse.  A refusal
 * leaves an earlier held-out set in place.                                                       */
int scs_set_test_sparse_device(scs_ctx* ctx, int64_t N, int64_t nnz,
                               const void* d_rowptr, int ptr_bytes, const void* d_colidx, int idx_bytes,
                               const void* d_val, int val_bytes, int val_f32, const double* y,
                               void* src_stream, int64_t N_global, int64_t row0);

/* ---- problem / regularizer / smoother ----------------------------------- */
int scs_set_loss(scs_ctx* ctx, int loss_kind, int ggn_kind, double scale);
/* λ: nlam = 1 (scalar) or 2 ([λ1, λ2] for "gl").  Box (indbox): lb/ub are
 * nbound = 1 scalars or nbound = m vectors (C_set).  Groups (gl): ind is the
 * 3 x ngroups Int matrix of get_P (column-major, 1-based start, end, weight;
 * prox-reg-utils.jl:27-62); the ranges must partition 1..m (any order) --
 * what get_Cmat (prox-reg-utils.jl:121-142) and the GL smoothers accept.    */
int scs_set_reg(scs_ctx* ctx, int reg_kind, const double* lam, int nlam,
                const double* lb, const double* ub, int64_t nbound,
                const int64_t* ind, int64_t ngroups);
/* Opt-in: reuse AᵀQA across steps when it does not depend on x -- least
 * squares under ProxNSCORE (hess_fx = c·AᵀA) or under ProxGGNSCORE with the
 * linear out_fn (J = A, Q = c·I).  The reference recomputes it every step
 * (prox-GGN-SCORE.jl:129, prox-N-SCORE.jl:55) and that stays the default;
 * with the cache on, later steps copy the (all-reduced) Gram of the first and
 * only the gradient is all-reduced.  Bit-identical results.  Costs one more
 * m_pad² fp64 buffer.                                                        */
int scs_set_gram_cache(scs_ctx* ctx, int on);
/* The compute arm of the fp32-vs-fp64 tolerance study (BASELINE configs[4]): on = 1 runs the
 * sparse products of fp32-stored values (scs_set_sparse val_f32 = 1) and the L-BFGS two-loop
 * recursion in fp32 ARITHMETIC (fp32 products, fp32 accumulation and dots, results widened to fp64);
 * everything else (f / η / step / prox / the m x m solves) stays fp64.  0 (default): fp64.      */
int scs_set_compute_f32(scs_ctx* ctx, int on);
/* The m x m (and the GGN sample-space (N+1)²) systems' solver.  SCS_SOLVER_DEFAULT: blocked
 * Cholesky on MFMA with the LU fallback (sample space: LU) -- equal to the reference's solves to
 * O(cond·eps).  SCS_SOLVER_REFERENCE: the reference's own factorizations -- Householder QR
 * (LAPACK dgeqrf / dlarfg / dlarft conventions, 128-column compact-WY panels) for ProxGGNSCORE's
 * `qr(JQJ) \ Je` and `qr(I + A) \ residual` (prox-GGN-SCORE.jl:126,131) and the LU for
 * ProxNSCORE's `(H + λ·Diagonal(Hr)) \ ∇q` (prox-N-SCORE.jl:70) -- for parity work on
 * ill-conditioned systems; slower (the QR panel is a column-by-column chain).                  */
#define SCS_SOLVER_DEFAULT 0
#define SCS_SOLVER_REFERENCE 1
int scs_set_solver(scs_ctx* ctx, int kind);
/* G of get_P(n, G, ind) (1-based, a permutation of 1..m): get_reg's group
 * term reads P.matrix*x = x[G] (prox-reg-utils.jl:31, regularizers.jl:24-27);
 * the prox (ProxL2) and the GL smoothers (Cmat) index x directly, as in the
 * reference.  Call after scs_set_reg(gl); the default is G = 1:m.           */
int scs_set_group_map(scs_ctx* ctx, const int64_t* G, int64_t ntotal);
/* Mh/nu as in the smoother struct (e.g. 2.0/2.6 for pseudo-Huber).  lb/ub
 * (indbox smoothers) follow bounds_sanity_check (prox-reg-utils.jl:144-158). */
int scs_set_smoother(scs_ctx* ctx, int kind, double mu, double Mh, double nu,
                     const double* lb, const double* ub, int64_t nbound);
/* model.L (nothing <=> has_L = 0); iterate!(…; α) sets L = 1/α.            */
int scs_set_L(scs_ctx* ctx, int has_L, double L);

/* ---- method  (init! / step!) -------------------------------------------- */
/* init!(method, x): select the method and reset its state (L-BFGS memory,
 * prox-L-BFGS-SCORE.jl:31-36).  mem = ProxLQNSCORE.m.                       */
int scs_method_init(scs_ctx* ctx, int method, int ss_type, int use_prox, int mem);
/* f(A, y, x) (iterate.jl:168).                                             */
int scs_eval_f(scs_ctx* ctx, const double* x, double* fval);
/* ∇f(A, y, x) (grad_fx; the ForwardDiff gradient of f when the user gives none,
 * prox-L-BFGS-SCORE.jl:84-97).                                              */
int scs_eval_grad(scs_ctx* ctx, const double* x, double* g);
/* get_reg(model, x, reg_name) (regularizers.jl:4-31).                      */
int scs_eval_reg(scs_ctx* ctx, const double* x, double* gval);
/* Minibatches: the collected DataLoader batch list of optim_loop!
 * (iterate.jl:124-146; utils.jl:18-25 get_data_loader / get_loader_subset).
 * Batch b is the local rows rows[offsets[b] .. offsets[b+1]) (0-based, any
 * order -- a shuffled loader's permutation is the caller's), gathered on the
 * device as the As, ys its step! sees (iterate.jl:205-207).  scs_iterate runs
 * the inner `for (i, sample) in enumerate(data)` loop over the registered
 * list; scs_select_batch(b) makes batch b the As, ys of the following scs_step
 * calls (b = -1: the full data).  f / get_reg / the histories always use the
 * full data (iterate.jl:168).  nbatch = 0 clears the list and frees every
 * batch view.  On several ranks the list holds GLOBAL rows: every rank passes
 * the same list and keeps the rows it owns (possibly none of a batch).  A
 * sparse A's batches are gathered dense (the reference's Matrix(As')) unless
 * scs_set_sparse_batches keeps them sparse.                                 */
int scs_set_batches(scs_ctx* ctx, const int64_t* rows, const int64_t* offsets, int64_t nbatch);
int scs_select_batch(scs_ctx* ctx, int64_t b);
/* Batch b of the registered list as a step sees it, gathered by scs_select_batch's own path: its
 * n_b x d rows widened to fp64 into A_out (column-major, leading dimension lda >= n_b; NULL skips
 * them) and its targets into Y_out (n_b, or n_b x nout column-major with leading dimension n_b;
 * NULL skips them).  A dense batch view only (a batch held as a sparse view under
 * scs_set_sparse_batches is refused); single-device contexts; the selection is left as found.    */
int scs_get_batch_data(scs_ctx* ctx, int64_t b, double* A_out, int64_t lda, double* Y_out);
/* Opt-in (default 0): under ProxLQNSCORE a minibatch of a sparse A stays sparse.  scs_select_batch
 * then builds a sparse view instead of the n_b x m_pad dense one: bit for bit the two blocked
 * copies scs_set_sparse would build from A[rows_b, :] (rows in batch order, a repeated row kept
 * twice, the stored value type unchanged), y[rows_b] and a workspace of its own -- so a step on the
 * view equals, bit for bit, the step of a context whose data is A[rows_b, :], y[rows_b].  ProxNSCORE
 * and ProxGGNSCORE want dense tiles and keep the dense view; scs_method_init with a method of the
 * other kind drops the views of the wrong kind.  A mode like scs_set_dense_f32: accepted at any
 * time, forwarded to the devices of a multi-device context; changing it drops the pooled batch
 * views (the registered list stays).  No effect on a dense A.
 * Views are kept per batch, in the order built, while their bytes stay within a budget: the bytes
 * the context's sparse data takes when scs_set_batches is called, or SCS_SPARSE_BATCH_CACHE_MB
 * (read at scs_set_batches; 0 keeps nothing).  Batches beyond the budget share one refillable view
 * per distinct size, rebuilt when it holds another batch.  A batch of more than 2^31 - 1 entries
 * is refused with SCS_ERR_ARG at scs_select_batch.                                              */
int scs_set_sparse_batches(scs_ctx* ctx, int on);
/* Opt-in (default 0): ProxGGNSCORE's sample-space branch (N + 1 <= m, prox-GGN-SCORE.jl:124-127) on a
 * sparse A forms P = A diag(1/Hr) Aᵀ from the nonzeros (sum_j cnt_j^2 multiply-adds over the columns'
 * entry counts) instead of a dense mirror of A, a dense Aᵀ copy and MFMA tiles.  P(k, i), k <= i, is
 * the sum over row i's entries in stored order of (h_j a_ij) a_kj; SCS_SPARSE_SAMPLE_KERNEL (0 plain
 * walk, the default; 1 packed walk) and SCS_SPARSE_GRAM_SHIFT change the kernel, not a bit of P.  The (N+1)^2
 * system, its LU or QR and the rest of the step are unchanged.  With scs_set_sparse_batches also on,
 * a batch with n_b + 1 <= m gets a sparse view under ProxGGNSCORE too (the pieces of a ProxLQNSCORE
 * view, the batch's CSR and a blocked copy of its CSC), so a step on it equals, bit for bit, the
 * step of a context holding A[rows_b, :], y[rows_b] with this mode on; the system scratch (2 n_b^2
 * doubles) is kept once per distinct batch size, not per view.  Batches with n_b + 1 > m and
 * ProxNSCORE keep the dense view.  A mode like scs_set_sparse_batches: accepted at any time,
 * forwarded to the devices of a multi-device context, changing it drops the pooled views.  It is
 * stored and has NO effect on a sharded or multi-device context (the sample-space branch across
 * ranks needs a dense A) and on a dense A.                                                      */
int scs_set_sparse_sample(scs_ctx* ctx, int on);
/* The sparse batch views: how many are held, their device bytes, and the views built since
 * scs_set_batches (a multi-device context: summed).  Any pointer may be NULL.                  */
int scs_batch_info(scs_ctx* ctx, int64_t* nviews, int64_t* view_bytes, int64_t* builds);
/* step!(method, model, reg_name, hμ, As, x, x_prev, ys, Cmat, iter;
 *       return_dx) (prox-N-SCORE.jl:34, prox-GGN-SCORE.jl:34,
 * prox-L-BFGS-SCORE.jl:69).  dx may be NULL.                               */
int scs_step(scs_ctx* ctx, const double* x, const double* x_prev, int64_t iter,
             double* x_new, double* dx, double* pri_res_norm);
/* step!(...; ∇fx) (iterate.jl:52-54): the caller's gradient replaces grad_f at every point the
 * step evaluates it (`grad_f = x -> ∇fx`, prox-N-SCORE.jl:66-68 and prox-L-BFGS-SCORE.jl:98-100:
 * ∇q, the BB step's ∇q_prev, the line search and the L-BFGS pair's γh); ProxGGNSCORE takes no ∇fx
 * (prox-GGN-SCORE.jl:34-135 never reads it).  grad_fx (m, host) NULL = scs_step.              */
int scs_step_grad(scs_ctx* ctx, const double* x, const double* x_prev, int64_t iter, const double* grad_fx,
                  double* x_new, double* dx, double* pri_res_norm);

/* ---- loop level  (iterate!(method, model, reg_name, hμ; max_epoch, x_tol,
 * f_tol) -> Solution, iterate.jl:56-76 / optim_loop! :100-267) ------------ */
/* History arrays of a Solution (iterate.jl:3-32), caller-owned, capacity
 * 2 * max_epoch + 1 each (times may be NULL): an epoch pushes its start entry
 * (:214) and, when a step stops on f_rel_error <= f_tol but the refreshed
 * f_rel_error no longer passes the test at :257, a terminate entry (:246)
 * too.  pri_res_norm[0] is the reference's `nothing` (NaN).                  */
typedef struct scs_history {
  double* obj;
  double* fval;
  double* pri_res_norm;
  double* rel;      /* rel_error: max(‖x − x*‖ / max(‖x*‖, 1), x_tol), or the
                       mean_square_error for reg "gl" (rel_kind = 1)       */
  double* objrel;   /* f_rel_error: max(|obj − obj*| / |obj*|, f_tol)       */
  double* times;    /* seconds since the start, millisecond resolution       */
  double* fvaltest; /* (r04) ftest(x) = f(Atest, ytest, x) of every pushed point when the
                       context holds test data (scs_set_test_*; iterate.jl:169-175,
                       utils.jl:55-57: one entry per obj entry); may be NULL.  Written only
                       through scs_iterate_ex, and only when test data is held  */
} scs_history;
/* optim_loop! on the device: init! + per epoch f(x) + get_reg(x) + one step!
 * per batch (the full batch, or the scs_set_batches list in order), the
 * reference's termination tests and history pushes.  x_star is
 * model.x (the comparison solution).  Outputs: final x, *n_hist entries,
 * *epochs (Solution.epochs).  Metrics / verbose printing stay in the host loop
 * (scsopt.iterate).  Requires scs_method_init.
 * ABI note (r05 -> r06): scs_iterate reads the six-field (r03) history and never writes
 * fvaltest; a context holding test data (scs_set_test_*) is refused with SCS_ERR_STATE --
 * callers built against the r04 seven-field struct call scs_iterate_ex instead.          */
int scs_iterate(scs_ctx* ctx, const double* x0, const double* x_star, int64_t max_epoch, double x_tol,
                double f_tol, int rel_kind, double* x_out, const scs_history* hist, int64_t* n_hist,
                int64_t* epochs);
/* The same loop with a sized history: hist_size = sizeof(scs_history) as the caller compiled it.
 * Fields beyond hist_size are taken as NULL, so a caller built against the six-field (r03) layout
 * is never written past its struct; scs_iterate itself is scs_iterate_ex with the six-field size
 * (it never touches fvaltest).  A context given exactly one of Atest / ytest (scs_set_test_data
 * with A or y NULL: the reference's xor case, iterate.jl:170-171) fails with SCS_ERR_REF
 * "UndefVarError: `ftest` not defined ..." at the loop's first stats push, as the reference's
 * first show_stat! (:201) does.                                                                 */
int scs_iterate_ex(scs_ctx* ctx, const double* x0, const double* x_star, int64_t max_epoch, double x_tol,
                   double f_tol, int rel_kind, double* x_out, const scs_history* hist, size_t hist_size,
                   int64_t* n_hist, int64_t* epochs);

/* ---- kernel-level entry points (parity tests) --------------------------- */
/* hμ.grad(Cmat, x), hμ.hess(Cmat, x)                                       */
int scs_smoother_eval(scs_ctx* ctx, const double* x, double* gr, double* Hr);
/* prox_step(invoke_prox(model, reg_name, z, 1 ./ Hr, λ, α))                */
int scs_prox_eval(scs_ctx* ctx, const double* z, const double* Hr, double lam,
                  double alpha, double* out);
/* G = Aᵀ diag(w) A (local rows; lower triangle + diagonal tiles), ldg >= m. */
int scs_gram_eval(scs_ctx* ctx, const double* w, double* G, int64_t ldg);
/* P = A diag(h) Aᵀ (h: m weights) of the selected batch or the full data, formed the way a
 * ProxGGNSCORE sample-space step forms it (from the nonzeros with scs_set_sparse_sample on a sparse
 * A, else Aᵀ copy + tiles), symmetrized; N x N into P, ldp >= N.  One rank.                     */
int scs_sample_gram_eval(scs_ctx* ctx, const double* h, double* P, int64_t ldp);
/* The sample-space system of a single-output ProxGGNSCORE step at x (prox-GGN-SCORE.jl:124-127), of
 * the selected batch or the full data, before the solve: x is uploaded, the smoother evaluated, then
 * the function the step itself calls runs the forward pass, P = A diag(1 ./ Hr) A', u = A (h .* lambda gr)
 * and the assembly -- on the context's own arm (a dense A, fp64 or fp32-stored; a sparse A from its
 * nonzeros with scs_set_sparse_sample, else from its dense mirror) and its cached A' copy, tile list
 * and scratch.  M of order n1 = N + 1 (column-major, ldm >= n1; nothing is written beyond order n1):
 * M[i][j] = delta_ij + q_i s_i s_j P_ij, M[i][N] = q_i s_i u_i, M[N][.] = e_N; b = [r; 1] (n1).  M or b
 * may be NULL.  SCS_ERR_STATE without data, loss, regularizer or smoother, on a multi-output context
 * (scs_multi_sample_system_eval serves it), or while the selected batch is held as ProxLQNSCORE's
 * sparse view (scs_set_sparse_batches: it keeps no rows for this system); SCS_ERR_ARG when N + 1 > m (the feature branch's shape:
 * scs_solve_eval / scs_gram_eval), without a GGN kind, on a callback loss (its J is the caller's), on
 * more than one rank, for a NULL x or ldm < n1.  A refusal leaves the context usable.               */
int scs_sample_system_eval(scs_ctx* ctx, const double* x, double* M, int64_t ldm, double* b);
/* out = Aᵀ v (local rows)                                                  */
int scs_gemv_t_eval(scs_ctx* ctx, const double* v, double* out);
/* out = A x (local rows)                                                   */
int scs_gemv_n_eval(scs_ctx* ctx, const double* x, double* out);

/* The m x m system of ProxNSCORE / ProxGGNSCORE, (Aᵀ diag(w) A + diag(dvec)) x = rhs
 * ((H + λ·Diagonal(Hr)) \ ∇q, prox-N-SCORE.jl:69-70; qr(JQJ) \ Je, prox-GGN-SCORE.jl:129-131),
 * through the step's own path: MFMA Gram, then the solver scs_set_solver selects (mode 0: by
 * default the hand-written Cholesky with the LU fallback), the hand-written LU alone (mode 1) or
 * the Householder QR (mode 2).  *used_lu = 1 when the LU ran.                                */
int scs_solve_eval(scs_ctx* ctx, const double* w, const double* dvec, const double* rhs, int mode,
                   double* x, int* used_lu);
/* Julia's `A \ b` for a dense square Matrix (LAPACK getrf + getrs) by the hand-written
 * blocked LU: A is row-major n x n; ipiv receives getrf's pivot rows (0-based), info its
 * first zero pivot (1-based; x is then not written, ipiv is dgetrf's).  A cooperative panel whose
 * candidate exchange timed out (a workgroup never became resident) is redone with the
 * column-step panels, the same factor bit for bit (scs_fallback_counts).
 * Needs a context only.                                                                    */
int scs_lu_eval(scs_ctx* ctx, int64_t n, const double* A, const double* b, double* x, int32_t* ipiv,
                int* info);
/* Test door: M x = b for a symmetric positive definite M by the hand-written Cholesky (LAPACK potrf +
 * potrs, uplo 'U') on buffers of its own, through the sequence a step runs on its Gram (the factor
 * with its redo after a late chain wait, the one-launch solves with their per-block redo; every
 * SCS_CHOL_* / SCS_SOLVE_* switch read per call; scs_fallback_counts).  M: column-major n x n, only
 * its upper triangle is read; padded to a multiple of 128 with a unit diagonal.  U (optional):
 * column-major n x n, its upper triangle receives the factor M = UᵀU and its strict lower triangle is
 * unspecified.  info: the first non-positive pivot (1-based, dpotrf's info; x is then not written).
 * Needs a context only.                                                                     */
int scs_chol_eval(scs_ctx* ctx, int64_t n, const double* M, const double* b, double* x, double* U,
                  int* info);
/* Test door: A x = b by the Householder QR (LAPACK geqrf conventions: beta = -sign(alpha)·‖·‖,
 * R(c, c) = beta, tau = 0 for a column that is already zero below the diagonal) on buffers of its
 * own, through the sequence of the sample-space system qr(I + A) \ residual (identity padding to a
 * multiple of 128, cooperative panels with their redo, the one-launch backward solve with its
 * per-block redo; every SCS_QR_* switch read per call; scs_fallback_counts).  A: row-major n x n.
 * R (optional): column-major n x n, its upper triangle receives R; the strict lower triangle is
 * unspecified (the reflectors' storage).  Needs a context only.                              */
int scs_qr_eval(scs_ctx* ctx, int64_t n, const double* A, const double* b, double* x, double* R);
/* Columns cols[0..ncols) of the local (dense) A, column-major N x ncols.                 */
int scs_get_columns(scs_ctx* ctx, const int64_t* cols, int64_t ncols, double* out);
/* The production Gram launch for weights w, with Aᵀv formed in the same pass where a step
 * fuses it (*fused = 1): entries G(ij[2k], ij[2k+1]) for k < n, and Aᵀv (m).              */
int scs_gram_atv_eval(scs_ctx* ctx, const double* w, const double* v, const int64_t* ij, int64_t n,
                      double* gvals, double* atv, int* fused);

/* Multi-output kernel-level doors (a dense A; K need not equal the context's nout).  X: d x K and
 * V: N x K, column-major; AX (N x K) = A X and ATV (d x K) = Aᵀ V, through the step's kernels.
 * 1 <= K <= 16.  Either pair (X, AX) / (V, ATV) may be NULL.  A sparse A held in the
 * scs_set_sparse_outputs mode is served by the context's own product arm with K = nout; any other
 * sparse context is refused with SCS_ERR_STATE.                                                    */
int scs_multi_products_eval(scs_ctx* ctx, int K, const double* X, const double* V, double* AX, double* ATV);
/* The assembled system of a multi-output context at x (nvar entries): G = JᵀQJ (nvar x nvar,
 * column-major, ldg >= nvar, both triangles) before λ diag Hr, g = vec(Aᵀ R) and *f = f(x).  Any
 * output may be NULL.                                                                              */
int scs_multi_system_eval(scs_ctx* ctx, const double* x, double* G, int64_t ldg, double* g, double* f);
/* The sample-space system of a multi-output ProxGGNSCORE step at x (scs_set_multi_sample), by the
 * step's own forward pass and assembly, before the solve: M of order n1 = N*nout + 1 (column-major,
 * ldm >= n1; nothing is written beyond order n1) and b (n1).  The regularizer and the smoother must
 * be set (h = 1 ./ Hr and lambda gr enter the system).  M or b may be NULL.  SCS_ERR_STATE without
 * nout or without the switch; SCS_ERR_ARG when N*nout + 1 > d*nout (the feature branch's shape) or
 * on a sparse A.  With timing on, the assembly launches (one per column block, and the tail) are
 * bracketed by events of their own and reported as step_ms / step_calls: no step runs in here.     */
int scs_multi_sample_system_eval(scs_ctx* ctx, const double* x, double* M, int64_t ldm, double* b);

/* ---- timing ------------------------------------------------------------- */
/* on = 0: off; 1: HIP events around every Gram / product / solve / step; n > 1: in
 * scs_iterate's pipelined ProxLQNSCORE loop only every n-th epoch's launches are bracketed
 * (each event record costs a dispatch gap), everything else as for 1.                      */
int scs_timing_enable(scs_ctx* ctx, int on);
int scs_timing_get(scs_ctx* ctx, scs_timing* out);
int scs_timing_reset(scs_ctx* ctx);
/* The kernels of the latest main Gram launch and sparse product launch, as rocprofv3 names them
 * ("" when none ran), NUL-terminated, truncated to the capacities.  On an fp32-stored dense A
 * (scs_set_dense_f32) the Gram is gram_sia_ta_kernel<float, ...> and `product` names the A x
 * kernel, gemv_n_kernel<float>.                                                              */
int scs_kernel_names(scs_ctx* ctx, char* gram, int64_t gram_cap, char* product, int64_t product_cap);
/* Fallbacks taken instead of failing (r06), counted since the context was created (a
 * multi-device context: summed over its devices).  counts[i] for i < n:
 *   SCS_FB_LU_COOP_REFUSED  LU panels whose cooperative launch the runtime refused (run as column steps)
 *   SCS_FB_LU_COOP_REDO     LU factorizations redone with column-step panels after the one-launch
 *                           panel's candidate exchange timed out (info = -1)
 *   SCS_FB_SOLVE_BLOCKS     Cholesky solves redone by per-block launches after a one-launch solve's
 *                           dependency wait gave up
 *   SCS_FB_QR_BLOCKS        QR backward solves redone by per-block launches (the same, for QR)
 *   SCS_FB_CHAIN_REDO       Cholesky factors redone with one launch per operation after a wait of
 *                           the dependency-driven chain (SCS_CHOL_DAG=1) gave up
 *   SCS_FB_PIPE_REDO        steps whose Gram + factor were redone unpipelined after a strip wait of
 *                           the pipelined factor (SCS_CHOL_PIPE) gave up
 *   SCS_FB_QR_COOP_REFUSED  QR panels whose cooperative launch the runtime refused (run as column steps)
 *   SCS_FB_QR_COOP_REDO     QR solves redone from the saved system with the per-column launches after
 *                           a one-launch panel's record exchange timed out
 * Each redo gives the bits of the mode it falls back to.                                   */
#define SCS_FB_LU_COOP_REFUSED 0
#define SCS_FB_LU_COOP_REDO 1
#define SCS_FB_SOLVE_BLOCKS 2
#define SCS_FB_QR_BLOCKS 3
#define SCS_FB_CHAIN_REDO 4
#define SCS_FB_PIPE_REDO 5
#define SCS_FB_QR_COOP_REFUSED 6
#define SCS_FB_QR_COOP_REDO 7
#define SCS_FB_N 8
int scs_fallback_counts(scs_ctx* ctx, int64_t* counts, int n);
/* Wait for all work on the context stream.                                 */
int scs_sync(scs_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* SCSOPT_H */

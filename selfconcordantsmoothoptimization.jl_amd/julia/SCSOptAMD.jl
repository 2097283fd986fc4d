# SCSOptAMD.jl -- Julia `ccall` binding of libscsopt (include/scsopt.h) for
# SelfConcordantSmoothOptimization.jl.  It adds a device-backed problem type
# whose objective and `step!` run on the MI355X; the reference's `iterate!` /
# `optim_loop!` (src/algorithms/iterate.jl) drive it unchanged.
#
# Shipped as the integration artefact; Julia is not installed in the build
# container or on the GPU box, so the executed host mirror is the Python
# package `scsopt` (same ABI, same call sequence).
module SCSOptAMD

using LinearAlgebra
using Random
using SparseArrays
using SelfConcordantSmoothOptimization
import SelfConcordantSmoothOptimization: step!, init!, ProximalMethod, ProxModel, is_interval_set

export DeviceProblem, configure!, iterate_device!, set_gram_cache!, set_solver!, rccl_unique_id, set_comm_rccl!,
       set_comm_callback!, set_test!, set_test_device!, set_compute_f32!, fallback_counts, data_info, samplewise,
       set_sparse_batches!, set_sparse_sample!, batch_info, set_multi_sample!, set_multi_batches!,
       set_multi_sparse_batches!,
       multi_sample_system

const lib = joinpath(@__DIR__, "..", "scsopt", "libscsopt.so")

const LOSS = Dict(:logistic_margin => 1, :logistic_ce => 2, :least_squares => 3, :quadratic => 4, :rosenbrock => 5,
                  :callback => 6, :softmax_ce => 8, :multi_least_squares => 9)
const GGN = Dict(nothing => 0, :sigmoid_ce => 1, :linear_ls => 2, :linear_softmax_ce => 4, :linear_multi_ls => 5)
const REG = Dict("l1" => 1, "l2" => 2, "indbox" => 3, "gl" => 4)
const SCS_ERR_REF = 5
const SCS_ERR_CALLBACK = 7

# the exception a loss callback raised on the host (the trampoline cannot throw through C):
# rethrown by chk, so a user error or the reference's MethodError reaches the caller as itself
const CB_EXCEPTION = Ref{Any}(nothing)

function chk(rc::Integer, ctx::Ptr{Cvoid})
    rc == 0 && return nothing
    if (rc == SCS_ERR_CALLBACK || rc == SCS_ERR_REF) && CB_EXCEPTION[] !== nothing
        err, CB_EXCEPTION[] = CB_EXCEPTION[], nothing
        throw(err)
    end
    msg = unsafe_string(ccall((:scs_last_error, lib), Cstring, (Ptr{Cvoid},), ctx))
    error(msg)   # SCS_ERR_REF carries the reference's own Base.error text
end

# ---- sample-wise losses outside the menu: f(A, y, x) = Σᵢ ℓ(yᵢ, aᵢᵀx) (SCS_LOSS_SAMPLEWISE) ----------
# A, y and every product with A stay on the device (any DeviceProblem door, row shards, minibatches,
# held-out rows); the caller's elementwise functions see z = A*x and y of the view in use.
#   host mode (device = false): value(z, y), d1(z, y), d2(z, y); link(z) = ŷ, link_d1(z), grad_fy(y, ŷ),
#     hess_fy(y, ŷ) (the diagonal) on Vector{Float64} views of the library's pinned buffers; each returns
#     n numbers (or a scalar, broadcast).
#   device mode (device = true): the same names receive the library's DEVICE pointers and its stream and
#     queue their own kernels on it: value(out, z, y, n, stream), d1(...), d2(...); link(ŷ_out, z, n, stream),
#     link_d1(s_out, z, n, stream), grad_fy(out, y, ŷ, n, stream), hess_fy(out, y, ŷ, n, stream).  Nothing
#     is synchronised around the call.
# Pass it where a loss Symbol goes: DeviceProblem(A, y, x0, samplewise(value; d1, d2), λ; ...).  No
# automatic differentiation: ProxLQNSCORE needs d1, ProxNSCORE d1 and d2, ProxGGNSCORE the four GGN pieces.
mutable struct Samplewise   # mutable: `user` is pointer_from_objref(sw), rooted by the model
    value::Function
    d1::Union{Function,Nothing}
    d2::Union{Function,Nothing}
    link::Union{Function,Nothing}
    link_d1::Union{Function,Nothing}
    grad_fy::Union{Function,Nothing}
    hess_fy::Union{Function,Nothing}
    device::Bool
end

function samplewise(value::Function, d1=nothing, d2=nothing; link=nothing, link_d1=nothing, grad_fy=nothing,
                    hess_fy=nothing, device::Bool=false)
    ggn = (link, link_d1, grad_fy, hess_fy)
    (any(isnothing, ggn) && !all(isnothing, ggn)) &&
        error("samplewise: link, link_d1, grad_fy and hess_fy go together (ProxGGNSCORE needs all four)")
    return Samplewise(value, d1, d2, link, link_d1, grad_fy, hess_fy, device)
end

has_ggn(sw::Samplewise) = all(!isnothing, (sw.link, sw.link_d1, sw.grad_fy, sw.hess_fy))
const LossSpec = Union{Symbol,Samplewise}

function samplewise_trampoline(user::Ptr{Cvoid}, what::Cint, n::Int64, zp::Ptr{Float64}, yp::Ptr{Float64},
                               vp::Ptr{Float64}, d1p::Ptr{Float64}, d2p::Ptr{Float64}, sp::Ptr{Float64},
                               stream::Ptr{Cvoid})::Cint
    sw = unsafe_pointer_to_objref(user)::Samplewise
    noad = " (no automatic differentiation on the device path)"
    try
        (what & 2) != 0 && sw.d1 === nothing && error("this method needs d1" * noad)
        (what & 4) != 0 && sw.d2 === nothing && error("ProxNSCORE needs d2" * noad)
        (what & 8) != 0 && !has_ggn(sw) && error("ProxGGNSCORE needs link, link_d1, grad_fy and hess_fy" * noad)
        if sw.device
            (what & 1) != 0 && sw.value(vp, zp, yp, n, stream)
            (what & 2) != 0 && sw.d1(d1p, zp, yp, n, stream)
            (what & 4) != 0 && sw.d2(d2p, zp, yp, n, stream)
            if (what & 8) != 0        # ŷ rests in the s area until r and q are formed from it
                sw.link(sp, zp, n, stream)
                sw.grad_fy(d1p, yp, sp, n, stream)
                sw.hess_fy(d2p, yp, sp, n, stream)
                sw.link_d1(sp, zp, n, stream)
            end
        else
            z, y = unsafe_wrap(Array, zp, n), unsafe_wrap(Array, yp, n)
            (what & 1) != 0 && (unsafe_wrap(Array, vp, n) .= sw.value(z, y))
            (what & 2) != 0 && (unsafe_wrap(Array, d1p, n) .= sw.d1(z, y))
            (what & 4) != 0 && (unsafe_wrap(Array, d2p, n) .= sw.d2(z, y))
            if (what & 8) != 0
                ŷ = sw.link(z)
                unsafe_wrap(Array, sp, n) .= sw.link_d1(z)
                unsafe_wrap(Array, d1p, n) .= sw.grad_fy(y, ŷ)
                unsafe_wrap(Array, d2p, n) .= sw.hess_fy(y, ŷ)
            end
        end
        return Cint(0)
    catch err
        CB_EXCEPTION[] = err
        return Cint(1)
    end
end

# register sw with the context; returns the (loss, ggn) kinds scs_set_loss takes
function bind_samplewise(ctx::Ptr{Cvoid}, sw::Samplewise)
    fp = @cfunction(samplewise_trampoline, Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                                                  Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}))
    chk(ccall((:scs_set_loss_samplewise, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint),
              ctx, fp, pointer_from_objref(sw), sw.device ? 1 : 0, has_ggn(sw) ? 1 : 0), ctx)
    return 7, (has_ggn(sw) ? 3 : 0)
end

mutable struct DeviceProblem <: ProxModel
    ctx::Ptr{Cvoid}
    A
    y
    x0::Vector{Float64}
    f
    λ
    Atest
    ytest
    L
    x::Vector{Float64}
    C_set
    P
    out_fn
    grad_fx
    hess_fx
    jac_yx
    grad_fy
    hess_fy
    name
end

# devices = [d0, d1, ...]: one process drives those GPUs (scs_create_multi) -- the library splits
# the rows across them, so a plain iterate! call uses the node's GPUs with no MPI (the reference's
# iterate! is one process, iterate.jl:56-76)
# device_exchange = :host: the group's exchange through host memory instead of RCCL
# (SCS_MULTI_HOST_EXCHANGE; devices may repeat a GPU)
const SCS_MULTI_HOST_EXCHANGE = Cint(1)
function create_ctx(device::Integer, devices=nothing, device_exchange::Symbol=:rccl)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    if devices === nothing
        rc = ccall((:scs_create, lib), Cint, (Cint, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), device, C_NULL, ctx)
        rc == 0 || error("scs_create failed ($rc)")
    else
        devs = Cint.(collect(devices))
        flags = device_exchange === :host ? SCS_MULTI_HOST_EXCHANGE : Cint(0)
        rc = ccall((:scs_create_multi_ex, lib), Cint, (Ptr{Cint}, Cint, Cint, Ref{Ptr{Cvoid}}), devs, length(devs),
                   flags, ctx)
        rc == 0 || error("scs_create_multi_ex($(devs), $(device_exchange)) failed ($rc)")
    end
    return ctx[]
end

function finish_problem(ctx, A, yv, x0, loss, λ, out_fn, scale, L, sol, C_set, P)
    if loss isa Samplewise   # its values arrive scaled (`scale` is not applied) and it carries its own GGN pieces
        out_fn === nothing || error("a sample-wise loss carries its own GGN pieces: no out_fn")
        lk, gk = bind_samplewise(ctx, loss)
        chk(ccall((:scs_set_loss, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Float64), ctx, lk, gk, 1.0), ctx)
    else
        chk(ccall((:scs_set_loss, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Float64), ctx, LOSS[loss], GGN[out_fn], scale), ctx)
    end
    model = DeviceProblem(ctx, A, yv, x0, nothing, λ, nothing, nothing, L, sol, C_set, P, out_fn,
                          loss isa Samplewise ? loss : nothing, nothing, nothing, nothing, nothing, nothing)
    # optim_loop! calls model.f(model.A, model.y, x) and, with held-out data, ftest(x) =
    # model.f(model.Atest, model.ytest, x) (iterate.jl:168,173): both evaluate on the device
    model.f = (A_, y_, x) -> (A_ !== nothing && A_ === model.Atest) ? devftest(model, x) : devf(model, x)
    finalizer(m_ -> ccall((:scs_destroy, lib), Cint, (Ptr{Cvoid},), m_.ctx), model)
    return model
end

# Problem(...; Atest, ytest) (problems.jl:27-28,67-68): the held-out rows go to the device; both
# are required.  One alone is the reference's xor case (iterate.jl:170-171): the model keeps what it
# was given (so the reference's own optim_loop! takes its xor path and raises by itself at :201), and
# the device records it, so iterate_device! logs the @info and raises UndefVarError(:ftest) as well.
# Sharded: this rank's rows of Ntest_global held-out rows starting at global row test_row0.
function set_test!(model::DeviceProblem, Atest, ytest; Ntest_global::Integer=0, test_row0::Integer=0,
                   val_f32::Bool=false)
    ctx = model.ctx
    chk(ccall((:scs_set_test_data, lib), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64),
              ctx, 0, C_NULL, 0, C_NULL, 0, 0), ctx)           # clear
    model.Atest, model.ytest = nothing, nothing
    (Atest === nothing && ytest === nothing) && return model
    if xor(Atest === nothing, ytest === nothing)
        one = zeros(1)
        chk(ccall((:scs_set_test_data, lib), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64),
                  ctx, 0, Atest === nothing ? C_NULL : pointer(one), 0, ytest === nothing ? C_NULL : pointer(one),
                  0, 0), ctx)
        model.Atest, model.ytest = Atest, ytest
        return model
    end
    yt = Vector{Float64}(vec(ytest))
    if model.grad_fx isa LossCallbacks                        # a callback loss: evaluated on the host
        model.grad_fx.test = (Atest, ytest)
        chk(ccall((:scs_set_test_callback, lib), Cint, (Ptr{Cvoid}, Cint), ctx, 1), ctx)
    elseif Atest isa SparseMatrixCSC
        At = SparseMatrixCSC(transpose(Atest))
        rowptr = Int64.(At.colptr .- 1); colidx = Int32.(At.rowval .- 1); val = Vector{Float64}(At.nzval)
        chk(ccall((:scs_set_test_sparse, lib), Cint,
                  (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Cint, Ptr{Float64}, Int64, Int64),
                  ctx, size(Atest, 1), nnz(Atest), rowptr, colidx, val, val_f32 ? 1 : 0, yt, Ntest_global,
                  test_row0), ctx)
    elseif Atest isa Matrix{Float32}                          # stored as fp32 on the device, as it is
        chk(ccall((:scs_set_test_data_f32, lib), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int64),
                  ctx, size(Atest, 1), Atest, size(Atest, 1), yt, Ntest_global, test_row0), ctx)
    else
        Am = Matrix{Float64}(Atest)
        chk(ccall((:scs_set_test_data, lib), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64),
                  ctx, size(Am, 1), Am, size(Am, 1), yt, Ntest_global, test_row0), ctx)
    end
    model.Atest, model.ytest = Atest, ytest
    return model
end

# Problem(A, y, x0, f, λ; ...) (problems.jl:61-81) with A on the device.  Row sharding: pass
# the local rows with N_global / row0, and attach a communicator (set_comm_rccl! /
# set_comm_callback!) before the first step.
function DeviceProblem(A::Matrix{Float64}, y::AbstractVector, x0::Vector{Float64}, loss::LossSpec, λ;
                       out_fn::Union{Symbol,Nothing}=nothing, scale::Float64=1.0 / size(A, 1),
                       L=nothing, sol::Vector{Float64}=zero(x0), C_set=nothing, P=nothing, device::Integer=0,
                       N_global::Integer=size(A, 1), row0::Integer=0, devices=nothing,
                       device_exchange::Symbol=:rccl, Atest=nothing,
                       ytest=nothing, Ntest_global::Integer=0, test_row0::Integer=0)
    ctx = create_ctx(device, devices, device_exchange)
    N, m = size(A)
    yv = Vector{Float64}(y)
    chk(ccall((:scs_set_data, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64),
              ctx, N, m, A, N, yv, N_global, row0), ctx)
    model = finish_problem(ctx, A, yv, x0, loss, λ, out_fn, scale, L, sol, C_set, P)
    return set_test!(model, Atest, ytest; Ntest_global, test_row0)
end

# A multi-output target (optim_loop! reads ny = size(model.y, 2), iterate.jl:106): Y is N x K, 2 <= K <= 16,
# x0 = vec(X0) with X0 d x K, loss :softmax_ce (out_fn :linear_softmax_ce) or :multi_least_squares
# (out_fn :linear_multi_ls).  scs_set_outputs goes before the data door, whose m is then A's column
# count d; A stays on the device as one N x d block (Matrix{Float32}: stored as fp32).  One device, one
# rank, the full batch; an Atest takes an Ntest x K ytest.  multi_sample = true: with N*K + 1 <= d*K
# ProxGGNSCORE runs the reference's sample-space branch on the device instead of being refused
# (scs_set_multi_sample).  multi_batches = true: iterate_device!(...; batch_size) / set_batches! are accepted
# (a dense A; the batch's rows of A and Y are gathered on the device) instead of being refused
# (scs_set_multi_batches).
function DeviceProblem(A::Union{Matrix{Float64},Matrix{Float32}}, Y::AbstractMatrix, x0::Vector{Float64},
                       loss::Symbol, λ; out_fn::Union{Symbol,Nothing}=nothing, scale::Float64=1.0 / size(A, 1),
                       L=nothing, sol::Vector{Float64}=zero(x0), C_set=nothing, P=nothing, device::Integer=0,
                       Atest=nothing, ytest=nothing, multi_sample::Bool=false, multi_batches::Bool=false)
    N, d = size(A)
    K = size(Y, 2)
    (size(Y, 1) == N && length(x0) == d * K) ||
        throw(DimensionMismatch("Y must be N x K and length(x0) = size(A, 2) * K"))
    ctx = create_ctx(device)
    multi_sample && chk(ccall((:scs_set_multi_sample, lib), Cint, (Ptr{Cvoid}, Cint), ctx, 1), ctx)
    multi_batches && chk(ccall((:scs_set_multi_batches, lib), Cint, (Ptr{Cvoid}, Cint), ctx, 1), ctx)
    chk(ccall((:scs_set_outputs, lib), Cint, (Ptr{Cvoid}, Cint), ctx, K), ctx)
    Ym = Matrix{Float64}(Y)
    if A isa Matrix{Float32}
        chk(ccall((:scs_set_data_f32, lib), Cint,
                  (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int64),
                  ctx, N, d, A, N, Ym, N, 0), ctx)
    else
        chk(ccall((:scs_set_data, lib), Cint,
                  (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64),
                  ctx, N, d, A, N, Ym, N, 0), ctx)
    end
    model = finish_problem(ctx, A, Ym, x0, loss, λ, out_fn, scale, L, sol, C_set, P)
    return set_test!(model, Atest, ytest)
end

# (nout, the length of x) of a context: (1, m) without scs_set_outputs
function get_outputs(model::DeviceProblem)
    k = Ref{Cint}(0); nv = Ref{Int64}(0)
    chk(ccall((:scs_get_outputs, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}), model.ctx, k, nv), model.ctx)
    return Int(k[]), Int(nv[])
end

# A*X (N x K) and A'*V (d x K) through the multi-output kernels (parity tests); 1 <= K <= 16
function multi_products(model::DeviceProblem, X::Matrix{Float64}, V::Matrix{Float64})
    N, K = size(V); d = size(X, 1)
    AX = zeros(N, K); ATV = zeros(d, K)
    chk(ccall((:scs_multi_products_eval, lib), Cint,
              (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              model.ctx, K, X, V, AX, ATV), model.ctx)
    return AX, ATV
end

# (J'QJ before λ*Diagonal(Hr), vec(A'R), f) of a multi-output problem at x, by the step's own path
function multi_system(model::DeviceProblem, x::Vector{Float64})
    n = length(x)
    G = zeros(n, n); g = zeros(n); f = Ref{Float64}(0.0)
    chk(ccall((:scs_multi_system_eval, lib), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ref{Float64}),
              model.ctx, x, G, n, g, f), model.ctx)
    return G, g, f[]
end

# ProxGGNSCORE's sample-space branch of a multi-output problem (N*K + 1 <= d*K, a dense A) on or off
# (scs_set_multi_sample; off by default: that shape is refused).  Stored without effect without nout.
function set_multi_sample!(model::DeviceProblem, on::Bool=true)
    chk(ccall((:scs_set_multi_sample, lib), Cint, (Ptr{Cvoid}, Cint), model.ctx, on ? 1 : 0), model.ctx)
    return model
end

# Minibatches of a multi-output problem (a dense A) on or off (scs_set_multi_batches; off by default:
# set_batches! is refused).  Stored without effect without nout; switching it off clears a registered list.
function set_multi_batches!(model::DeviceProblem, on::Bool=true)
    chk(ccall((:scs_set_multi_batches, lib), Cint, (Ptr{Cvoid}, Cint), model.ctx, on ? 1 : 0), model.ctx)
    return model
end

# Minibatches of a multi-output problem on a sparse A on or off (scs_set_multi_sparse_batches; off by
# default: set_batches! asks for a dense A).  set_multi_batches! stays the gate.  Stored without effect
# without nout or on a dense A; switching it off clears a sparse multi-output problem's registered list.
function set_multi_sparse_batches!(model::DeviceProblem, on::Bool=true)
    chk(ccall((:scs_set_multi_sparse_batches, lib), Cint, (Ptr{Cvoid}, Cint), model.ctx, on ? 1 : 0), model.ctx)
    return model
end

# (M, b) of the sample-space system a multi-output ProxGGNSCORE step solves at x (multi_sample = true;
# the regularizer and the smoother set): M of order N*K + 1, rows and columns (i, k) = i + N*k
function multi_sample_system(model::DeviceProblem, x::Vector{Float64})
    K, _ = get_outputs(model)
    n1 = size(model.y, 1) * K + 1
    M = zeros(n1, n1); b = zeros(n1)
    chk(ccall((:scs_multi_sample_system_eval, lib), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}),
              model.ctx, x, M, n1, b), model.ctx)
    return M, b
end

# A::Matrix{Float32} (A::DataTupleOrArray2 admits it, problems.jl:61-62; with x::Vector{Float64} Julia
# promotes every product to Float64): the rows are stored as fp32 on the device as they are -- half
# the memory of A, fp64 arithmetic, bit for bit what Float64.(A) gives (scs_set_data_f32).  An
# Atest::Matrix{Float32} is stored the same way; any other dense Atest is rounded to fp32 on the device.
function DeviceProblem(A::Matrix{Float32}, y::AbstractVector, x0::Vector{Float64}, loss::LossSpec, λ;
                       out_fn::Union{Symbol,Nothing}=nothing, scale::Float64=1.0 / size(A, 1),
                       L=nothing, sol::Vector{Float64}=zero(x0), C_set=nothing, P=nothing, device::Integer=0,
                       N_global::Integer=size(A, 1), row0::Integer=0, devices=nothing,
                       device_exchange::Symbol=:rccl, Atest=nothing,
                       ytest=nothing, Ntest_global::Integer=0, test_row0::Integer=0)
    ctx = create_ctx(device, devices, device_exchange)
    N, m = size(A)
    yv = Vector{Float64}(y)
    chk(ccall((:scs_set_data_f32, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int64),
              ctx, N, m, A, N, yv, N_global, row0), ctx)
    model = finish_problem(ctx, A, yv, x0, loss, λ, out_fn, scale, L, sol, C_set, P)
    return set_test!(model, Atest, ytest; Ntest_global, test_row0)
end

# A that is already on the GPU (scs_set_data_device): `ptr` is device memory on `device`, element (n, j)
# of the N x m matrix at ptr[n*strides[1] + j*strides[2]] (strides in elements, one of them 1), elements
# of type `elem` (Float64 or Float32).  A column-major ROCArray{T,2} is strides = (1, size(A, 1)), its
# default here; a row-major buffer is strides = (m, 1).  The matrix is re-tiled on the device: no host
# copy.  dense_f32 alone decides the stored type (a Float32 source with dense_f32 = false is widened, a
# Float64 one with dense_f32 = true rounded on the device).  y: a host vector, or a Ptr{Cvoid} to N
# device Float64.  stream: the HIP stream that produced A (C_NULL: the caller has synchronised).  The
# call returns with the copy done, so A may be freed.  Single-device contexts only.
# Written against the header; never executed (no Julia / AMDGPU.jl on the build machines).
device_y(y::Ptr{Cvoid}, N) = (y, convert(Ptr{Float64}, y))
function device_y(y::AbstractVector, N)
    yv = Vector{Float64}(y)
    length(yv) == N || throw(DimensionMismatch("y has $(length(yv)) entries, A has $N rows"))
    return (yv, pointer(yv))
end

function DeviceProblem(ptr::Ptr{Cvoid}, N::Integer, m::Integer, y::Union{AbstractVector,Ptr{Cvoid}},
                       x0::Vector{Float64}, loss::LossSpec, λ;
                       elem::Type=Float64, strides::Tuple{Integer,Integer}=(1, N), dense_f32::Bool=false,
                       stream::Ptr{Cvoid}=C_NULL,
                       out_fn::Union{Symbol,Nothing}=nothing, scale::Float64=1.0 / N,
                       L=nothing, sol::Vector{Float64}=zero(x0), C_set=nothing, P=nothing, device::Integer=0,
                       N_global::Integer=N, row0::Integer=0)
    (elem === Float64 || elem === Float32) || throw(ArgumentError("elem is Float64 or Float32"))
    length(x0) == m || throw(DimensionMismatch("x0 has $(length(x0)) entries, A has $m columns"))
    ctx = create_ctx(device, nothing, :rccl)
    chk(ccall((:scs_set_dense_f32, lib), Cint, (Ptr{Cvoid}, Cint), ctx, dense_f32 ? 1 : 0), ctx)
    yroot, yp = device_y(y, N)
    GC.@preserve yroot chk(ccall((:scs_set_data_device, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}, Int64, Int64),
              ctx, N, m, ptr, sizeof(elem), strides[1], strides[2], yp, stream, N_global, row0), ctx)
    return finish_problem(ctx, nothing, y isa Ptr ? nothing : yroot, x0, loss, λ, out_fn, scale, L, sol, C_set, P)
end

# held-out rows from device memory (scs_set_test_data_device), as DeviceProblem(ptr, ...) takes A
function set_test_device!(model::DeviceProblem, ptr::Ptr{Cvoid}, Ntest::Integer,
                          ytest::Union{AbstractVector,Ptr{Cvoid}}; elem::Type=Float64,
                          strides::Tuple{Integer,Integer}=(1, Ntest), stream::Ptr{Cvoid}=C_NULL,
                          Ntest_global::Integer=0, test_row0::Integer=0)
    (elem === Float64 || elem === Float32) || throw(ArgumentError("elem is Float64 or Float32"))
    yroot, yp = device_y(ytest, Ntest)
    GC.@preserve yroot chk(ccall((:scs_set_test_data_device, lib), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}, Int64, Int64),
              model.ctx, Ntest, ptr, sizeof(elem), strides[1], strides[2], yp, stream, Ntest_global, test_row0),
        model.ctx)
    return model
end

# (element bytes of the dense A: 8 or 4, bytes of that block, device bytes the context holds)
function data_info(model::DeviceProblem)
    eb = Ref{Cint}(0); ab = Ref{Int64}(0); cb = Ref{Int64}(0)
    chk(ccall((:scs_data_info, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}, Ref{Int64}), model.ctx, eb, ab, cb),
        model.ctx)
    return Int(eb[]), ab[], cb[]
end

# A::SparseMatrixCSC (README.md:105 builds it with sprandn): its CSC arrays are the column copy;
# the row copy is the CSC of the transpose.  0-based indices on the C side.
function DeviceProblem(A::SparseMatrixCSC{Float64}, y::AbstractVector, x0::Vector{Float64}, loss::LossSpec, λ;
                       out_fn::Union{Symbol,Nothing}=nothing, scale::Float64=1.0 / size(A, 1),
                       L=nothing, sol::Vector{Float64}=zero(x0), C_set=nothing, P=nothing, device::Integer=0,
                       val_f32::Bool=false, N_global::Integer=size(A, 1), row0::Integer=0, Atest=nothing,
                       ytest=nothing, Ntest_global::Integer=0, test_row0::Integer=0,
                       sparse_batches::Bool=false, sparse_sample::Bool=false)
    ctx = create_ctx(device)
    sparse_batches && chk(ccall((:scs_set_sparse_batches, lib), Cint, (Ptr{Cvoid}, Cint), ctx, 1), ctx)
    sparse_sample && chk(ccall((:scs_set_sparse_sample, lib), Cint, (Ptr{Cvoid}, Cint), ctx, 1), ctx)
    N, m = size(A)
    yv = Vector{Float64}(y)
    At = SparseMatrixCSC(transpose(A))
    rowptr = Int64.(At.colptr .- 1); colidx = Int32.(At.rowval .- 1); val = Vector{Float64}(At.nzval)
    colptr = Int64.(A.colptr .- 1);  rowidx = Int32.(A.rowval .- 1);  valT = Vector{Float64}(A.nzval)
    chk(ccall((:scs_set_sparse, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Cint, Ptr{Float64}, Int64, Int64),
              ctx, N, m, nnz(A), rowptr, colidx, val, colptr, rowidx, valT, val_f32 ? 1 : 0, yv, N_global, row0),
        ctx)
    model = finish_problem(ctx, A, yv, x0, loss, λ, out_fn, scale, L, sol, C_set, P)
    return set_test!(model, Atest, ytest; Ntest_global, test_row0, val_f32)
end

# A sparse A that is already on the GPU (scs_set_sparse_device): the CSR triple of a
# CuSparseMatrixCSR-style matrix as three device pointers -- rowptr (N + 1 entries of ptr_type), colidx
# (nnz entries of idx_type, 0-BASED: subtract 1 on the device from a Julia-side 1-based array) and val
# (nnz entries of elem) -- with their element types (Int32 / Int64, Float32 / Float64).  The library
# validates the arrays, builds the CSC copy and both blocked copies on the device: no host copy.
# val_f32 alone decides the stored type.  Unsorted rows and duplicate entries are kept as they are.
# y, stream: as for the dense device method above.  Single-device contexts only.
# Written against the header; never executed (no Julia / AMDGPU.jl on the build machines).
csr_width(T::Type) = (T === Int32 || T === Int64) ? Cint(sizeof(T)) :
                     throw(ArgumentError("pointer / index type is Int32 or Int64"))
val_width(T::Type) = (T === Float32 || T === Float64) ? Cint(sizeof(T)) :
                     throw(ArgumentError("elem is Float64 or Float32"))

function DeviceProblem(rowptr::Ptr{Cvoid}, colidx::Ptr{Cvoid}, val::Ptr{Cvoid}, N::Integer, m::Integer,
                       nnz::Integer, y::Union{AbstractVector,Ptr{Cvoid}}, x0::Vector{Float64}, loss::LossSpec, λ;
                       ptr_type::Type=Int64, idx_type::Type=Int32, elem::Type=Float64, val_f32::Bool=false,
                       stream::Ptr{Cvoid}=C_NULL,
                       out_fn::Union{Symbol,Nothing}=nothing, scale::Float64=1.0 / N,
                       L=nothing, sol::Vector{Float64}=zero(x0), C_set=nothing, P=nothing, device::Integer=0,
                       N_global::Integer=N, row0::Integer=0)
    length(x0) == m || throw(DimensionMismatch("x0 has $(length(x0)) entries, A has $m columns"))
    pb, ib, vb = csr_width(ptr_type), csr_width(idx_type), val_width(elem)
    ctx = create_ctx(device, nothing, :rccl)
    yroot, yp = device_y(y, N)
    GC.@preserve yroot chk(ccall((:scs_set_sparse_device, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint,
               Ptr{Float64}, Ptr{Cvoid}, Int64, Int64),
              ctx, N, m, nnz, rowptr, pb, colidx, ib, val, vb, val_f32 ? 1 : 0, yp, stream, N_global, row0), ctx)
    return finish_problem(ctx, nothing, y isa Ptr ? nothing : yroot, x0, loss, λ, out_fn, scale, L, sol, C_set, P)
end

# A multi-output target on a sparse A (scs_set_sparse_outputs; opt-in): Y is N x K, x0 = vec(X0) with
# X0 d x K, loss :softmax_ce / :multi_least_squares as for the dense method above.  With
# sparse_outputs = true the sparse doors accept A under scs_set_outputs and the products A*X, A'*R read
# the nonzeros once for all K columns; without it the library refuses, naming the switch.  One device,
# one rank; a sparse Atest takes an Ntest x K ytest.  Minibatches need multi_batches = true (the gate,
# scs_set_multi_batches) and multi_sparse_batches = true (scs_set_multi_sparse_batches, which lifts the
# dense-A requirement): a batch is then a densified view or, with sparse_batches = true under ProxLQNSCORE,
# a sparse K-column view.
function DeviceProblem(A::SparseMatrixCSC{Float64}, Y::AbstractMatrix, x0::Vector{Float64}, loss::Symbol, λ;
                       sparse_outputs::Bool=false, out_fn::Union{Symbol,Nothing}=nothing,
                       scale::Float64=1.0 / size(A, 1), L=nothing, sol::Vector{Float64}=zero(x0), C_set=nothing,
                       P=nothing, device::Integer=0, val_f32::Bool=false, Atest=nothing, ytest=nothing,
                       multi_sample::Bool=false, multi_batches::Bool=false, sparse_batches::Bool=false,
                       multi_sparse_batches::Bool=false)
    N, d = size(A)
    K = size(Y, 2)
    (size(Y, 1) == N && length(x0) == d * K) ||
        throw(DimensionMismatch("Y must be N x K and length(x0) = size(A, 2) * K"))
    ctx = create_ctx(device)
    multi_sample && chk(ccall((:scs_set_multi_sample, lib), Cint, (Ptr{Cvoid}, Cint), ctx, 1), ctx)
    multi_batches && chk(ccall((:scs_set_multi_batches, lib), Cint, (Ptr{Cvoid}, Cint), ctx, 1), ctx)
    sparse_batches && chk(ccall((:scs_set_sparse_batches, lib), Cint, (Ptr{Cvoid}, Cint), ctx, 1), ctx)
    multi_sparse_batches &&
        chk(ccall((:scs_set_multi_sparse_batches, lib), Cint, (Ptr{Cvoid}, Cint), ctx, 1), ctx)
    chk(ccall((:scs_set_sparse_outputs, lib), Cint, (Ptr{Cvoid}, Cint), ctx, sparse_outputs ? 1 : 0), ctx)
    chk(ccall((:scs_set_outputs, lib), Cint, (Ptr{Cvoid}, Cint), ctx, K), ctx)
    Ym = Matrix{Float64}(Y)
    At = SparseMatrixCSC(transpose(A))
    rowptr = Int64.(At.colptr .- 1); colidx = Int32.(At.rowval .- 1); val = Vector{Float64}(At.nzval)
    colptr = Int64.(A.colptr .- 1);  rowidx = Int32.(A.rowval .- 1);  valT = Vector{Float64}(A.nzval)
    chk(ccall((:scs_set_sparse, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Cint, Ptr{Float64}, Int64, Int64),
              ctx, N, d, nnz(A), rowptr, colidx, val, colptr, rowidx, valT, val_f32 ? 1 : 0, Ym, N, 0), ctx)
    model = finish_problem(ctx, A, Ym, x0, loss, λ, out_fn, scale, L, sol, C_set, P)
    return set_test!(model, Atest, ytest; val_f32)
end

# ... and from a device CSR (the method above with three device pointers): m is A's column count d, Y a
# host N x K matrix.
function DeviceProblem(rowptr::Ptr{Cvoid}, colidx::Ptr{Cvoid}, val::Ptr{Cvoid}, N::Integer, m::Integer,
                       nnz::Integer, Y::AbstractMatrix, x0::Vector{Float64}, loss::Symbol, λ;
                       sparse_outputs::Bool=false, ptr_type::Type=Int64, idx_type::Type=Int32, elem::Type=Float64,
                       val_f32::Bool=false, stream::Ptr{Cvoid}=C_NULL,
                       out_fn::Union{Symbol,Nothing}=nothing, scale::Float64=1.0 / N,
                       L=nothing, sol::Vector{Float64}=zero(x0), C_set=nothing, P=nothing, device::Integer=0)
    K = size(Y, 2)
    (size(Y, 1) == N && length(x0) == m * K) ||
        throw(DimensionMismatch("Y must be N x K and length(x0) = m * K"))
    pb, ib, vb = csr_width(ptr_type), csr_width(idx_type), val_width(elem)
    ctx = create_ctx(device, nothing, :rccl)
    chk(ccall((:scs_set_sparse_outputs, lib), Cint, (Ptr{Cvoid}, Cint), ctx, sparse_outputs ? 1 : 0), ctx)
    chk(ccall((:scs_set_outputs, lib), Cint, (Ptr{Cvoid}, Cint), ctx, K), ctx)
    Ym = Matrix{Float64}(Y)
    GC.@preserve Ym chk(ccall((:scs_set_sparse_device, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint,
               Ptr{Float64}, Ptr{Cvoid}, Int64, Int64),
              ctx, N, m, nnz, rowptr, pb, colidx, ib, val, vb, val_f32 ? 1 : 0, pointer(Ym), stream, N, 0), ctx)
    return finish_problem(ctx, nothing, Ym, x0, loss, λ, out_fn, scale, L, sol, C_set, P)
end

# CSR held-out rows from device memory (scs_set_test_sparse_device), as the method above takes A
function set_test_sparse_device!(model::DeviceProblem, rowptr::Ptr{Cvoid}, colidx::Ptr{Cvoid}, val::Ptr{Cvoid},
                                 Ntest::Integer, nnz::Integer, ytest::Union{AbstractVector,Ptr{Cvoid}};
                                 ptr_type::Type=Int64, idx_type::Type=Int32, elem::Type=Float64,
                                 val_f32::Bool=false, stream::Ptr{Cvoid}=C_NULL, Ntest_global::Integer=0,
                                 test_row0::Integer=0)
    pb, ib, vb = csr_width(ptr_type), csr_width(idx_type), val_width(elem)
    yroot, yp = device_y(ytest, Ntest)
    GC.@preserve yroot chk(ccall((:scs_set_test_sparse_device, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint,
               Ptr{Float64}, Ptr{Cvoid}, Int64, Int64),
              model.ctx, Ntest, nnz, rowptr, pb, colidx, ib, val, vb, val_f32 ? 1 : 0, yp, stream, Ntest_global,
              test_row0), model.ctx)
    return model
end

# Minibatches of a sparse A stay sparse under ProxLQNSCORE (scs_set_sparse_batches; off by default:
# the batch is then the reference's Matrix(As')).  Changing the mode drops the pooled batch views.
function set_sparse_batches!(model::DeviceProblem, on::Bool=true)
    chk(ccall((:scs_set_sparse_batches, lib), Cint, (Ptr{Cvoid}, Cint), model.ctx, on ? 1 : 0), model.ctx)
    return model
end

# ProxGGNSCORE's sample-space branch (N + 1 <= m) on a sparse A forms P = A diag(1/Hr) Aᵀ from the nonzeros
# (scs_set_sparse_sample; off by default: a dense mirror, an Aᵀ copy and MFMA tiles).  With
# set_sparse_batches! also on, its batches with n_b + 1 <= m become sparse views.  No effect on a
# sharded context or a dense A.  Changing the mode drops the pooled batch views.
function set_sparse_sample!(model::DeviceProblem, on::Bool=true)
    chk(ccall((:scs_set_sparse_sample, lib), Cint, (Ptr{Cvoid}, Cint), model.ctx, on ? 1 : 0), model.ctx)
    return model
end

# (sparse batch views held, their device bytes, views built since the batch list was registered)
function batch_info(model::DeviceProblem)
    nv = Ref{Int64}(0); vb = Ref{Int64}(0); bd = Ref{Int64}(0)
    chk(ccall((:scs_batch_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), model.ctx, nv, vb, bd),
        model.ctx)
    return nv[], vb[], bd[]
end

# the device's CSC copy of a sparse A, back on the host as a SparseMatrixCSC (values widened)
function get_sparse_csc(model::DeviceProblem, N::Integer, m::Integer)
    n = Ref{Int64}(0)
    chk(ccall((:scs_get_nnz, lib), Cint, (Ptr{Cvoid}, Ref{Int64}), model.ctx, n), model.ctx)
    colptr = zeros(Int64, m + 1); rowidx = zeros(Int32, max(n[], 1)); valT = zeros(Float64, max(n[], 1))
    chk(ccall((:scs_get_sparse_csc, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}),
              model.ctx, colptr, rowidx, valT), model.ctx)
    return SparseMatrixCSC(N, m, colptr .+ 1, Int64.(rowidx[1:n[]]) .+ 1, valT[1:n[]])
end

# ---- user losses outside the menu: the reference's own keyword callbacks ------------------
# Problem(x0, f, λ; grad_fx, hess_fx) (problems.jl:44-59) / Problem(A, y, x0, f, λ; grad_fx,
# hess_fx) (:61-81) evaluated on the host (SCS_LOSS_CALLBACK); the smoother, the solve, damping,
# prox and the loop stay on the device.  No ForwardDiff fallback: ProxLQNSCORE needs grad_fx,
# ProxNSCORE grad_fx and hess_fx.
mutable struct LossCallbacks   # mutable: `user` is pointer_from_objref(cbs), rooted by the model
    f::Function
    grad_fx::Union{Function,Nothing}
    hess_fx::Union{Function,Nothing}
    out_fn::Union{Function,Nothing}  # ProxGGNSCORE pieces (prox-GGN-SCORE.jl:44-49)
    jac_yx::Union{Function,Nothing}
    grad_fy::Union{Function,Nothing}
    hess_fy::Union{Function,Nothing}
    data::Union{Tuple,Nothing}       # (A, y) of a data problem: the closures take (A, y, x)
    nout::Int64                      # length(vec(ŷ)): the Jacobian rows (0: no GGN pieces)
    test::Union{Tuple,Nothing}       # (Atest, ytest): f(Atest, ytest, x) for SCS_CB_FTEST
end

# J, r and diag(Q) of the step: a non-diagonal Q is eigen-rotated (J̃ = VᵀJ, r̃ = Vᵀr, q = λ),
# which leaves JᵀQJ, Jᵀr and the sample-space system of ggn_score_step unchanged
function ggn_pieces!(out::Vector{Float64}, cbs::LossCallbacks, x::Vector{Float64})
    A, y = cbs.data
    n, m = cbs.nout, length(x)
    ŷ = cbs.out_fn(A, x)
    J = Matrix{Float64}(reshape(cbs.jac_yx(A, y, ŷ, x), n, m))
    r = Vector{Float64}(vec(cbs.grad_fy(A, y, ŷ)))
    Q = cbs.hess_fy(A, y, ŷ)
    if Q isa AbstractVector || isdiag(Q)
        q = Q isa AbstractVector ? Vector{Float64}(Q) : Vector{Float64}(diag(Q))
    else
        E = eigen(Symmetric(Matrix{Float64}((Q + Q') / 2)))
        J, r, q = E.vectors' * J, E.vectors' * r, E.values
    end
    out[1:n*m] .= vec(J)
    out[n*m+1:n*(m+1)] .= r
    out[n*(m+1)+1:n*(m+2)] .= q
    return nothing
end

function loss_trampoline(user::Ptr{Cvoid}, what::Cint, xp::Ptr{Float64}, m::Int64, outp::Ptr{Float64})::Cint
    cbs = unsafe_pointer_to_objref(user)::LossCallbacks
    try
        x = copy(unsafe_wrap(Array, xp, m))
        args = cbs.data === nothing ? (x,) : (cbs.data..., x)
        if what == 0
            unsafe_store!(outp, Float64(cbs.f(args...)))
        elseif what == 1
            cbs.grad_fx === nothing && error("this method needs grad_fx (no automatic differentiation on the device path)")
            copyto!(unsafe_wrap(Array, outp, m), cbs.grad_fx(args...))
        elseif what == 3
            ggn_pieces!(unsafe_wrap(Array, outp, cbs.nout * (m + 2)), cbs, x)
        elseif what == 4                                   # SCS_CB_FTEST (iterate.jl:173)
            unsafe_store!(outp, Float64(cbs.f(cbs.test..., x)))
        elseif what == 5                                   # SCS_CB_GRAD_X: ProxGGNSCORE's grad_f =
            cbs.grad_fx === nothing && error("this method needs grad_fx (no automatic differentiation on the device path)")
            if !applicable(cbs.grad_fx, x)                 # x -> model.grad_fx(x) (prox-GGN-SCORE.jl:58-59)
                CB_EXCEPTION[] = MethodError(cbs.grad_fx, (x,))
                return Cint(2)                             # SCS_CB_NO_METHOD -> SCS_ERR_REF
            end
            copyto!(unsafe_wrap(Array, outp, m), cbs.grad_fx(x))
        else
            cbs.hess_fx === nothing && error("ProxNSCORE needs hess_fx (no automatic differentiation on the device path)")
            copyto!(unsafe_wrap(Array, outp, m * m), vec(Matrix{Float64}(cbs.hess_fx(args...))))   # column-major
        end
        return Cint(0)
    catch err
        CB_EXCEPTION[] = err
        return Cint(1)
    end
end

function callback_problem(cbs::LossCallbacks, x0::Vector{Float64}, λ, L, sol, C_set, P, device)
    ctx = create_ctx(device)
    m = length(x0)
    chk(ccall((:scs_set_data, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64),
              ctx, 0, m, C_NULL, 0, C_NULL, 0, 0), ctx)
    model = finish_problem(ctx, nothing, nothing, x0, :callback, λ, nothing, 1.0, L, sol, C_set, P)
    model.grad_fx = cbs                         # rooted with the model: `user` points at it
    fp = @cfunction(loss_trampoline, Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Ptr{Float64}))
    chk(ccall((:scs_set_loss_callback, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
              ctx, fp, pointer_from_objref(cbs), cbs.nout), ctx)
    return model
end

DeviceProblem(x0::Vector{Float64}, f::Function, λ; grad_fx=nothing, hess_fx=nothing, L=nothing,
              sol::Vector{Float64}=zero(x0), C_set=nothing, P=nothing, device::Integer=0) =
    callback_problem(LossCallbacks(f, grad_fx, hess_fx, nothing, nothing, nothing, nothing, nothing, 0, nothing),
                     x0, λ, L, sol, C_set, P, device)

# y may be a matrix (ny > 1 outputs, iterate.jl:105-107): out_fn / jac_yx / grad_fy / hess_fy see it as is
function DeviceProblem(A::AbstractMatrix, y::AbstractVecOrMat, x0::Vector{Float64}, f::Function, λ; grad_fx=nothing,
                       hess_fx=nothing, out_fn=nothing, jac_yx=nothing, grad_fy=nothing, hess_fy=nothing,
                       L=nothing, sol::Vector{Float64}=zero(x0), C_set=nothing, P=nothing, device::Integer=0,
                       Atest=nothing, ytest=nothing)
    ggn = all(!isnothing, (out_fn, jac_yx, grad_fy, hess_fy))
    nout = ggn ? Int64(length(out_fn(A, x0))) : 0
    cbs = LossCallbacks(f, grad_fx, hess_fx, out_fn, jac_yx, grad_fy, hess_fy, (A, y), nout, nothing)
    model = callback_problem(cbs, x0, λ, L, sol, C_set, P, device)
    return set_test!(model, Atest, ytest)
end

# ---- row sharding (SURVEY.md §8e): one process per GPU, A's rows split across them ---------
# libscsopt's own RCCL communicator: rank 0 draws the id, the caller hands the 128 bytes to
# every rank (MPI.jl's Bcast!, a shared file ...), every rank then calls set_comm_rccl!.
function rccl_unique_id()
    id = zeros(UInt8, 128)
    rc = ccall((:scs_rccl_unique_id, lib), Cint, (Ptr{Cvoid},), id)
    rc == 0 || error("scs_rccl_unique_id failed ($rc)")
    return id
end

function set_comm_rccl!(model::DeviceProblem, rank::Integer, nranks::Integer, id::Vector{UInt8})
    length(id) == 128 || error("an RCCL unique id is 128 bytes")
    chk(ccall((:scs_set_comm_rccl, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}), model.ctx, rank, nranks, id),
        model.ctx)
    return model
end

# Or any all-reduce the host owns: `sum!(buf::Ptr{Float64}, count::Int64, stream::Ptr{Cvoid})`
# sums `count` doubles in place across ranks on the device (e.g. an RCCL call through
# AMDGPU.jl); the payload lives in a device buffer of reduce_buffer_size doubles registered here.
const CALLBACKS = Dict{Ptr{Cvoid},Any}()

function allreduce_trampoline(buf::Ptr{Cvoid}, count::Int64, stream::Ptr{Cvoid}, user::Ptr{Cvoid})::Cint
    try
        CALLBACKS[user](Ptr{Float64}(buf), count, stream)
        return Cint(0)
    catch
        return Cint(1)
    end
end

function set_comm_callback!(model::DeviceProblem, rank::Integer, nranks::Integer, sum!::Function,
                            dev_buf::Ptr{Cvoid}=C_NULL)
    CALLBACKS[model.ctx] = sum!
    fn = @cfunction(allreduce_trampoline, Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}))
    chk(ccall((:scs_set_comm, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
              model.ctx, rank, nranks, fn, model.ctx), model.ctx)
    if dev_buf != C_NULL
        n = Ref{Int64}(0)
        chk(ccall((:scs_reduce_buffer_size, lib), Cint, (Ptr{Cvoid}, Ref{Int64}), model.ctx, n), model.ctx)
        chk(ccall((:scs_set_reduce_buffer, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), model.ctx, dev_buf, n[]),
            model.ctx)
    end
    return model
end

function devf(model::DeviceProblem, x::Vector{Float64})
    out = Ref{Float64}(0.0)
    chk(ccall((:scs_eval_f, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}), model.ctx, x, out), model.ctx)
    return out[]
end

function devftest(model::DeviceProblem, x::Vector{Float64})
    out = Ref{Float64}(0.0)
    chk(ccall((:scs_eval_ftest, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}), model.ctx, x, out), model.ctx)
    return out[]
end

"""configure!(model, reg_name, hμ): push reg_name/λ/C_set/P and the smoother to the device."""
function configure!(model::DeviceProblem, reg_name::String, hμ)
    haskey(REG, reg_name) || error("reg_name not valid.")
    lam = Float64.(collect(model.λ isa Number ? (model.λ,) : model.λ))
    lb = ub = Float64[]; nb = 0
    ind = Int64[]; ng = 0
    if reg_name == "indbox"
        lb, ub = cset_bounds(model.C_set); nb = length(lb)
    elseif reg_name == "gl"
        ind = Int64.(vec(model.P.ind)); ng = size(model.P.ind, 2)     # column-major 3 x G, 1-based
    end
    chk(ccall((:scs_set_reg, lib), Cint,
              (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Int64),
              model.ctx, REG[reg_name], lam, length(lam), lb, ub, nb, ind, ng), model.ctx)
    if reg_name == "gl"                                  # P.matrix*x = x[G] in get_reg
        G = Int64.(model.P.G)
        chk(ccall((:scs_set_group_map, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64), model.ctx, G, length(G)),
            model.ctx)
    end
    kind, slb, sub = smoother_kind(hμ, model)
    chk(ccall((:scs_set_smoother, lib), Cint,
              (Ptr{Cvoid}, Cint, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Int64),
              model.ctx, kind, hμ.μ, hμ.Mh, hμ.ν, slb, sub, length(slb)), model.ctx)
    chk(ccall((:scs_set_L, lib), Cint, (Ptr{Cvoid}, Cint, Float64), model.ctx, model.L === nothing ? 0 : 1,
              model.L === nothing ? 0.0 : Float64(model.L)), model.ctx)
    return model
end

# C_set -> (lb, ub) exactly as prox_step(::scaled_proximal_indbox) reads it
# (prox-operators.jl:34-46): an interval, a tuple of intervals, or a (lb, ub) pair / vector.
function cset_bounds(C_set)
    C_set === nothing && error("indbox needs model.C_set")
    if is_interval_set(C_set)
        lb, ub = C_set isa Tuple ? ([minimum.(C_set)...], [maximum.(C_set)...]) : (minimum(C_set), maximum(C_set))
    else
        lb, ub = C_set[1], C_set[2]
    end
    return Float64.(vcat(lb)), Float64.(vcat(ub))
end

# The IndBox smoothers keep their bounds only in the closures they build
# (phuber-smooth.jl:59-65, exponential-smooth.jl:28-34, log-exp-smooth.jl:28-34:
# `grad = (Cmat,x) -> huber_grad_indbox(x; μ=mu, lb=lb, ub=ub)`), so the captured `lb` / `ub`
# are read off the closure object (a closure's captures are its fields); model.C_set is the
# fallback for a hand-built smoother whose closure captured other names.
function indbox_bounds(hμ, model)
    g = hμ.grad
    if hasfield(typeof(g), :lb) && hasfield(typeof(g), :ub)
        return Float64.(vcat(getfield(g, :lb))), Float64.(vcat(getfield(g, :ub)))
    end
    return cset_bounds(model.C_set)
end

# smoother struct -> (kind, lb, ub)
function smoother_kind(hμ, model)
    T = typeof(hμ)
    T <: PHuberSmootherL1L2 && return (1, Float64[], Float64[])
    T <: PHuberSmootherIndBox && return (2, indbox_bounds(hμ, model)...)
    T <: PHuberSmootherGL && return (3, Float64[], Float64[])
    T <: ExponentialSmootherIndBox && return (4, indbox_bounds(hμ, model)...)
    T <: LogExpSmootherIndBox && return (5, indbox_bounds(hμ, model)...)
    T <: OsBaSmootherL1L2 && return (6, Float64[], Float64[])
    T <: OsBaSmootherGL && return (7, Float64[], Float64[])
    error("smoother $(T) has no device implementation")
end

# Opt-in reuse of the x-independent AᵀQA of least squares across steps (scs_set_gram_cache);
# the reference recomputes it every step (prox-GGN-SCORE.jl:129) and that stays the default.
set_gram_cache!(model::DeviceProblem, on::Bool=true) =
    chk(ccall((:scs_set_gram_cache, lib), Cint, (Ptr{Cvoid}, Cint), model.ctx, on ? 1 : 0), model.ctx)

# The reference's own factorizations (scs_set_solver): Householder QR for ProxGGNSCORE's systems
# (prox-GGN-SCORE.jl:126,131), LU for ProxNSCORE's -- the default is Cholesky with the LU fallback.
set_solver!(model::DeviceProblem, reference::Bool=true) =
    chk(ccall((:scs_set_solver, lib), Cint, (Ptr{Cvoid}, Cint), model.ctx, reference ? 1 : 0), model.ctx)

# The compute arm of the fp32-vs-fp64 study (BASELINE configs[4]): fp32 arithmetic in the sparse
# products of fp32-stored values (val_f32 = true) and the L-BFGS two-loop (scs_set_compute_f32).
set_compute_f32!(model::DeviceProblem, on::Bool=true) =
    chk(ccall((:scs_set_compute_f32, lib), Cint, (Ptr{Cvoid}, Cint), model.ctx, on ? 1 : 0), model.ctx)

# The fallbacks taken instead of failing since the problem's context was created (scs_fallback_counts;
# SCS_FB_* in include/scsopt.h, in that order), as name => count.
const FALLBACKS = (:lu_coop_refused, :lu_coop_redo, :solve_blocks, :qr_blocks, :chain_redo, :pipe_redo,
                   :qr_coop_refused, :qr_coop_redo)
function fallback_counts(model::DeviceProblem)
    out = zeros(Int64, length(FALLBACKS))
    chk(ccall((:scs_fallback_counts, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Cint), model.ctx, out, length(out)),
        model.ctx)
    return Dict(zip(FALLBACKS, out))
end

method_code(m) = m isa ProxNSCORE ? 1 : m isa ProxGGNSCORE ? 2 : m isa ProxLQNSCORE ? 3 : error("unknown method")

# init!(method, x) for device problems (prox-L-BFGS-SCORE.jl:31-36)
function init_device!(method::ProximalMethod, model::DeviceProblem)
    mem = method isa ProxLQNSCORE ? method.m : 0
    chk(ccall((:scs_method_init, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint),
              model.ctx, method_code(method), method.ss_type, method.use_prox, mem), model.ctx)
end

# step! on a DeviceProblem: the whole per-iteration work runs in libscsopt.
function step!(method::ProximalMethod, model::DeviceProblem, reg_name, hμ, As, x, x_prev, ys, Cmat, iter;
               ∇fx=nothing, return_dx=false)
    # the device holds the rows: a minibatch As from the reference's loader cannot be mapped back
    # to them, so minibatches go through iterate_device!(...; batch_size) (scs_set_batches)
    As === nothing || size(As, 1) == size(model.A, 1) ||
        error("minibatch As on a DeviceProblem: use iterate_device!(...; batch_size, shuffle_batch)")
    x_new = similar(x); dx = similar(x); pri = Ref{Float64}(0.0)
    # ∇fx (iterate.jl:52-54): grad_f = x -> ∇fx inside the step (prox-L-BFGS-SCORE.jl:98-100)
    g = ∇fx === nothing ? C_NULL : Vector{Float64}(vec(∇fx))
    g === C_NULL || length(g) == length(x) || error("∇fx must have length(x) entries")
    chk(ccall((:scs_step_grad, lib), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
              model.ctx, x, x_prev, iter, g, x_new, dx, pri), model.ctx)
    return return_dx ? (x_new, dx, pri[]) : (x_new, pri[])
end

# The collected loader batches of optim_loop! (iterate.jl:124-146, utils.jl:14-25) as 0-based
# row lists: ceil(N/b) consecutive runs of the (randperm-shuffled) sample order, the last one
# partial; slice_samples keeps only sample 1 (max_iter stays 1); local_max_iter truncates.
# `nothing` = the one full batch.
function loader_batches(N::Int, batch_size, slice_samples::Bool, shuffle_batch::Bool, local_max_iter)
    batch_size !== nothing && slice_samples && (slice_samples = false)
    max_iter = batch_size !== nothing ? Int(ceil(N / batch_size)) : 1
    iend = (local_max_iter !== nothing && Int(floor(local_max_iter)) > 0) ?
           min(Int(floor(local_max_iter)), max_iter) : max_iter
    slice_samples && return [Int64[i - 1] for i in 1:min(iend, N)]
    batch_size === nothing && return nothing
    order = shuffle_batch ? randperm(N) .- 1 : collect(0:N-1)
    return [Int64.(order[(i-1)*batch_size+1:min(i * batch_size, N)]) for i in 1:iend]
end

function set_batches!(model::DeviceProblem, batches)
    if batches === nothing || isempty(batches)
        chk(ccall((:scs_set_batches, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int64),
                  model.ctx, C_NULL, C_NULL, 0), model.ctx)
        return
    end
    rows = reduce(vcat, batches)
    offs = Int64[0; cumsum(length.(batches))]
    chk(ccall((:scs_set_batches, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int64),
              model.ctx, rows, offs, length(batches)), model.ctx)
end

# iterate!(method, model::DeviceProblem, reg_name, hμ; max_epoch, x_tol, f_tol, batch_size, ...):
# optim_loop! (iterate.jl:100-267) as ONE ccall (scs_iterate) -- no per-epoch host round trips;
# minibatches are gathered on the device from the registered row lists (scs_set_batches).
# Returns the reference's Solution (iterate.jl:3-32); pri_res_norm[1] is `nothing` as there.
# The rows of all ranks (scs_get_dims): the loader's N on a row-sharded problem.
function global_rows(model::DeviceProblem)
    Ng = Ref{Int64}(0)
    chk(ccall((:scs_get_dims, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ref{Int64}, Ptr{Int64}),
              model.ctx, C_NULL, C_NULL, Ng, C_NULL), model.ctx)
    Ng[]
end

# Row-sharded minibatches: every rank registers the same GLOBAL batch list and keeps its own rows
# of each batch; `bcast` (e.g. `b -> MPI.bcast(b, 0, comm)`) hands rank 0's shuffled list to all.
function iterate_device!(method::ProximalMethod, model::DeviceProblem, reg_name::String, hμ;
                         α=nothing, batch_size=nothing, slice_samples=false, shuffle_batch=true,
                         max_epoch=1000, local_max_iter=nothing, x_tol=1e-10, f_tol=1e-10, bcast=identity)
    local_max_iter === nothing || (max_epoch = 1)      # iterate.jl:66
    α === nothing || (model.L = 1 / α)                 # iterate.jl:113-115
    batches = (batch_size !== nothing || slice_samples) ?
              bcast(loader_batches(Int(global_rows(model)), batch_size, slice_samples, shuffle_batch,
                                   local_max_iter)) : nothing
    set_batches!(model, batches)
    try
        return iterate_registered!(method, model, reg_name, hμ, max_epoch, x_tol, f_tol)
    finally
        batches === nothing || set_batches!(model, nothing)
    end
end

function iterate_registered!(method, model, reg_name, hμ, max_epoch, x_tol, f_tol)
    configure!(model, reg_name, hμ)
    init_device!(method, model)
    cap = 2 * max_epoch + 1                           # scsopt.h: up to two pushes per epoch
    obj, fval, pri, rel, objrel, tms, ftst = (Vector{Float64}(undef, cap) for _ in 1:7)
    has_test = model.Atest !== nothing && model.ytest !== nothing   # iterate.jl:169-175: Solution.fvaltest
    xor_test = xor(model.Atest === nothing, model.ytest === nothing)
    xor_test && @info "Both input (Atest) and target (ytest) data are required for testing the model, but only one of these has been provided.\nWill skip testing..."
    hist = (pointer(obj), pointer(fval), pointer(pri), pointer(rel), pointer(objrel), pointer(tms),
            has_test ? pointer(ftst) : Ptr{Float64}(C_NULL))
    x_out = similar(model.x0); nh = Ref{Int64}(0); ep = Ref{Int64}(0)
    GC.@preserve obj fval pri rel objrel tms ftst begin
        rc = ccall((:scs_iterate_ex, lib), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Float64, Cint, Ptr{Float64},
                    Ref{NTuple{7,Ptr{Float64}}}, Csize_t, Ref{Int64}, Ref{Int64}),
                   model.ctx, model.x0, model.x, max_epoch, x_tol, f_tol, reg_name == "gl" ? 1 : 0, x_out,
                   hist, sizeof(NTuple{7,Ptr{Float64}}), nh, ep)
        # the xor case fails at the first stats push, as show_stat! does at iterate.jl:201
        (xor_test && rc == SCS_ERR_REF) && throw(UndefVarError(:ftest))
        chk(rc, model.ctx)
    end
    n = nh[]
    pris = Any[isnan(pri[i]) && i == 1 ? nothing : pri[i] for i in 1:n]
    return Solution(x_out, obj[1:n], fval[1:n], pris, has_test ? ftst[1:n] : [], rel[1:n], objrel[1:n], Dict(),
                    tms[1:n], ep[], model)
end

end # module

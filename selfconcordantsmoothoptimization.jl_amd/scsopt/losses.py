"""Loss kinds: the closed-form stand-ins for the reference's user callbacks.

In the reference a problem carries Julia closures ``f(A, y, x)`` (and, for
ProxGGNSCORE, ``out_fn(A, x)`` plus a second method ``f(y, ŷ)``) whose
derivatives come from ForwardDiff or from user-supplied ``grad_fx``/
``hess_fx``/``jac_yx``/``grad_fy``/``hess_fy`` (problems.jl:21-40,61-81).
On the device the callbacks become a fixed menu of loss kinds evaluated by
HIP kernels; each kind states the reference expression it reproduces.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional


@dataclass(frozen=True)
class Loss:
    """x-form objective f(A, y, x)."""
    kind: str
    scale: float = 1.0

    def __repr__(self):
        return f"{self.kind}(scale={self.scale!r})"


@dataclass(frozen=True)
class OutFn:
    """out_fn(A, x) paired with its ŷ-form loss f(y, ŷ) (ProxGGNSCORE)."""
    kind: str
    scale: float = 1.0


def logistic_margin(scale: float = 1.0) -> Loss:
    """f(A,y,x) = scale*sum(log.(1 .+ exp.(-y .* (A*x))))   (test/test_algs.jl:9, README.md:113)."""
    return Loss("logistic_margin", float(scale))


def logistic_ce(scale: float = 1.0) -> Loss:
    """f(A,y,x) = f(y, σ(A*x)) with the cross-entropy f(y,ŷ) of test/test_algs.jl:10."""
    return Loss("logistic_ce", float(scale))


def least_squares(scale: float = 1.0) -> Loss:
    """f(A,y,x) = 0.5*sum((A*x .- y).^2)*scale   (README.md:212-214 with scale = 1/m)."""
    return Loss("least_squares", float(scale))


def quadratic() -> Loss:
    """f(A,y,x) = 1/2*(x'*(A*x)) + (y'*x)   (test/test_algs.jl:90; A is m x m)."""
    return Loss("quadratic", 1.0)


def rosenbrock() -> Loss:
    """f(x) = Σ 100(x[i+1]-x[i]^2)^2 + (1-x[i])^2   (README.md:49; ProblemGeneric, no data)."""
    return Loss("rosenbrock", 1.0)


@dataclass(frozen=True, eq=False)
class CallbackLoss(Loss):
    """The caller's own closures, evaluated on the host (SCS_LOSS_CALLBACK)."""
    f: Optional[Callable] = field(default=None, repr=False)
    grad_fx: Optional[Callable] = field(default=None, repr=False)
    hess_fx: Optional[Callable] = field(default=None, repr=False)
    out_fn: Optional[Callable] = field(default=None, repr=False)
    jac_yx: Optional[Callable] = field(default=None, repr=False)
    grad_fy: Optional[Callable] = field(default=None, repr=False)
    hess_fy: Optional[Callable] = field(default=None, repr=False)

    @property
    def has_ggn(self):
        return None not in (self.out_fn, self.jac_yx, self.grad_fy, self.hess_fy)


def callback(f, grad_fx=None, hess_fx=None, *, out_fn=None, jac_yx=None, grad_fy=None,
             hess_fy=None) -> CallbackLoss:
    """A user loss outside the menu: Problem(x0, f, λ; grad_fx, hess_fx) (problems.jl:44-59, f(x))
    or Problem(A, y, x0, f, λ; grad_fx, hess_fx, out_fn, jac_yx, grad_fy, hess_fy) (:61-81,
    f(A, y, x)), the reference's own keyword callbacks (prox-N-SCORE.jl:49-56,
    prox-L-BFGS-SCORE.jl:85-91, prox-GGN-SCORE.jl:44-49).  They run on the host with NumPy
    arrays; the smoother, the Gram / m x m solve or the sample-space system, damping, prox and the
    loop stay on the device.  There is no automatic differentiation here (the reference falls
    back to ForwardDiff): ProxLQNSCORE needs grad_fx, ProxNSCORE grad_fx and hess_fx,
    ProxGGNSCORE out_fn(A, x), jac_yx(A, y, ŷ, x) (rows = vec(ŷ), column-major for a
    multi-output ŷ), grad_fy(A, y, ŷ) and hess_fy(A, y, ŷ) (a vector = diagonal Q, or a
    symmetric matrix) plus grad_fx for the line search."""
    return CallbackLoss("callback", 1.0, f, grad_fx, hess_fx, out_fn, jac_yx, grad_fy, hess_fy)


@dataclass(frozen=True, eq=False)
class SamplewiseLoss(Loss):
    """f(A, y, x) = Σᵢ ℓ(yᵢ, aᵢᵀx) with the caller's elementwise ℓ and derivatives
    (SCS_LOSS_SAMPLEWISE): A, y and every product with A stay on the device."""
    value: Optional[Callable] = field(default=None, repr=False)
    d1: Optional[Callable] = field(default=None, repr=False)
    d2: Optional[Callable] = field(default=None, repr=False)
    link: Optional[Callable] = field(default=None, repr=False)
    link_d1: Optional[Callable] = field(default=None, repr=False)
    grad_fy: Optional[Callable] = field(default=None, repr=False)
    hess_fy: Optional[Callable] = field(default=None, repr=False)
    device: bool = False

    @property
    def has_ggn(self):
        return None not in (self.link, self.link_d1, self.grad_fy, self.hess_fy)


def samplewise(value, d1=None, d2=None, *, link=None, link_d1=None, grad_fy=None, hess_fy=None,
               device=False) -> SamplewiseLoss:
    """A loss outside the menu of the form f(A, y, x) = Σᵢ ℓ(yᵢ, zᵢ), z = A*x (Poisson, Huber, squared
    hinge, probit, any GLM), usable wherever a menu kind is: the device keeps A (dense fp64 / fp32,
    sparse, device arrays, row shards, minibatches, held-out rows) and every product with it; the
    callables see z and y and return one number per sample.
      value(z, y) -> ℓ(yᵢ, zᵢ) (scaled as f is: no scale is applied), d1(z, y) -> ∂ℓ/∂z,
      d2(z, y) -> ∂²ℓ/∂z²;
      for ProxGGNSCORE ŷᵢ = φ(zᵢ), f = Σ ℓ(yᵢ, ŷᵢ): link(z) -> ŷ, link_d1(z) -> dŷ/dz,
      grad_fy(y, ŷ) -> ∂f/∂ŷ, hess_fy(y, ŷ) -> ∂²f/∂ŷ² (the diagonal of hess_fy), all four or none.
    There is no automatic differentiation on the device path: ProxLQNSCORE (and every ∇f) needs d1,
    ProxNSCORE d1 and d2, ProxGGNSCORE the four GGN pieces (d1 as well for its line search).
    device=False: the callables get NumPy arrays (z crosses to the host per call, y once per view).
    device=True: they get torch tensors that alias the library's device buffers, on the context's
    stream (torch imported before scsopt); nothing crosses, the library does not synchronise."""
    if not callable(value):
        raise TypeError("samplewise(value, ...): value(z, y) must be callable")
    for name, fn in (("d1", d1), ("d2", d2), ("link", link), ("link_d1", link_d1), ("grad_fy", grad_fy),
                     ("hess_fy", hess_fy)):
        if fn is not None and not callable(fn):
            raise TypeError(f"samplewise: {name} must be callable or None")
    ggn = (link, link_d1, grad_fy, hess_fy)
    if any(g is not None for g in ggn) and any(g is None for g in ggn):
        raise ValueError("samplewise: link, link_d1, grad_fy and hess_fy go together (ProxGGNSCORE needs all four)")
    return SamplewiseLoss("samplewise", 1.0, value, d1, d2, link, link_d1, grad_fy, hess_fy, bool(device))


@dataclass(frozen=True)
class MultiLoss(Loss):
    """A loss with nout = K outputs on one A: x = vec(X), X d x K column-major; Y is N x K."""
    nout: int = 2

    def __repr__(self):
        return f"{self.kind}(nout={self.nout}, scale={self.scale!r})"


@dataclass(frozen=True)
class MultiOutFn(OutFn):
    """out_fn(A, x) = A*X of a multi-output loss with its ŷ-form f(Y, ŷ) (ProxGGNSCORE)."""
    nout: int = 2


def _check_nout(nout):
    k = int(nout)
    if k != nout or not 2 <= k <= 16:
        raise ValueError(f"nout = {nout!r} is outside 2..16")
    return k


def softmax_ce(nout: int, scale: float = 1.0) -> MultiLoss:
    """Multinomial logistic regression on the device: x = vec(X), X d x nout (entry (j, l) at j + d*l),
    Z = A*X, P = softmax of the rows of Z, f(A, Y, x) = -scale*sum(Y .* log.(P)) with Y N x nout (rows
    need not be one-hot).  ∇f = vec(Aᵀ R), R = scale*(s_i P - Y), s_i = Σ_k Y_ik; block (k, l) of the
    Hessian is Aᵀ diag(scale s_i (δ_kl P_ik - P_ik P_il)) A.  A stays on the device as one N x d block."""
    return MultiLoss("softmax_ce", float(scale), _check_nout(nout))


def multi_least_squares(nout: int, scale: float = 1.0) -> MultiLoss:
    """f(A, Y, x) = 0.5*scale*sum((A*X .- Y).^2), X = reshape(x, d, nout), Y N x nout."""
    return MultiLoss("multi_least_squares", float(scale), _check_nout(nout))


def linear_softmax_ce(nout: int, scale: float = 1.0) -> MultiOutFn:
    """out_fn(A, x) = A*X (the logits) with f(Y, ŷ) = -scale*sum(Y .* log.(softmax(ŷ))): J = I ⊗ A and
    Q is block-diagonal per sample, scale s_i (diag(P_i) - P_i P_iᵀ)."""
    return MultiOutFn("linear_softmax_ce", float(scale), _check_nout(nout))


def linear_multi_ls(nout: int, scale: float = 1.0) -> MultiOutFn:
    """out_fn(A, x) = A*X with f(Y, ŷ) = 0.5*scale*sum((ŷ .- Y).^2): J = I ⊗ A, Q = scale*I."""
    return MultiOutFn("linear_multi_ls", float(scale), _check_nout(nout))


def sigmoid_ce(scale: float = 1.0) -> OutFn:
    """Mfunc(A,x) = 1 ./ (1 .+ exp.(-A*x)) with f(y,ŷ) = -scale*sum(y.*log.(ŷ) .+ (1 .- y).*log.(1 .- ŷ))
    (test/test_algs.jl:10-11, README.md:135-139)."""
    return OutFn("sigmoid_ce", float(scale))


def linear_ls(scale: float = 1.0) -> OutFn:
    """out_fn(A,x) = A*x with f(y,ŷ) = 0.5*sum((ŷ .- y).^2)*scale   (README.md:233-239)."""
    return OutFn("linear_ls", float(scale))


def ggn_kind(out_fn: Optional[OutFn]):
    return None if out_fn is None else out_fn.kind

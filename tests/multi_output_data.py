"""Shared data of the multi-output tests (test_multi_output_host.py, test_gpu_multi_output.py): the two
multi-output losses as NumPy closures for the oracle's / the device's callback route, in the general
form (rows of Y need not be one-hot: s_i = Σ_k Y_ik), and the problem generator.

x = vec(X), X d x K column-major (entry (j, l) at j + d·l); Y is N x K; Z = A X; P = softmax of the
rows of Z; c = scale.

  softmax_ce           f = -c Σ_i Σ_k Y_ik log P_ik     R = c (s_i P_ik - Y_ik)   Q_i = c s_i (diag(P_i) - P_i P_iᵀ)
  multi_least_squares  f = 0.5 c ‖A X - Y‖²_F           R = c (Z - Y)             Q_i = c I

∇f = vec(Aᵀ R); block (k, l) of ∇²f = JᵀQJ is Aᵀ diag(w_kl) A, w_kl,i = Q_i[k, l]; J = I_K ⊗ A
(rows (i, k) = i + N k, columns (j, l) = j + d l, the order losses.callback documents)."""
import numpy as np

KINDS = ("softmax_ce", "multi_least_squares")


def probs(Z):
    E = np.exp(Z - Z.max(axis=1, keepdims=True))
    return E / E.sum(axis=1, keepdims=True)


def log_probs(Z):
    S = Z - Z.max(axis=1, keepdims=True)
    return S - np.log(np.exp(S).sum(axis=1, keepdims=True))


def q_blocks(kind, Y, Z, c):
    """The per-sample K x K blocks of Q: an N x K x K array."""
    N, K = Z.shape
    if kind == "multi_least_squares":
        return np.broadcast_to(c * np.eye(K), (N, K, K)).copy()
    P = probs(Z)
    s = Y.sum(axis=1)
    return c * s[:, None, None] * (P[:, :, None] * np.eye(K)[None] - P[:, :, None] * P[:, None, :])


def closures(kind, d, K, c):
    """dict of f, grad_fx, hess_fx (the block formula), out_fn, jac_yx, grad_fy, hess_fy (dense); every
    closure takes the A, Y it is called with (the held-out set reuses f)."""
    assert kind in KINDS

    def X_of(x):
        return np.asarray(x, dtype=np.float64).reshape(d, K, order="F")

    def resid(Y, Z):
        if kind == "softmax_ce":
            return c * (Y.sum(axis=1, keepdims=True) * probs(Z) - Y)
        return c * (Z - Y)

    def f(A, Y, x):
        Z = A @ X_of(x)
        if kind == "softmax_ce":
            return -c * float(np.sum(Y * log_probs(Z)))
        return 0.5 * c * float(np.sum((Z - Y) ** 2))

    def grad_fx(A, Y, x):
        return (A.T @ resid(Y, A @ X_of(x))).ravel(order="F")

    def hess_fx(A, Y, x):
        Q = q_blocks(kind, Y, A @ X_of(x), c)
        H = np.zeros((d * K, d * K))
        for k in range(K):
            for l in range(K):
                H[k * d:(k + 1) * d, l * d:(l + 1) * d] = A.T @ (Q[:, k, l][:, None] * A)
        return H

    def out_fn(A, x):
        return A @ X_of(x)

    def jac_yx(A, Y, Z, x):
        return np.kron(np.eye(K), A)

    def grad_fy(A, Y, Z):
        return resid(Y, Z)

    def hess_fy(A, Y, Z):
        N = Z.shape[0]
        Q = q_blocks(kind, Y, Z, c)
        D = np.zeros((N * K, N * K))
        for i in range(N):
            idx = i + N * np.arange(K)
            D[np.ix_(idx, idx)] = Q[i]
        return D

    return dict(f=f, grad_fx=grad_fx, hess_fx=hess_fx, out_fn=out_fn, jac_yx=jac_yx, grad_fy=grad_fy,
                hess_fy=hess_fy)


def oracle_loss(O, kind, d, K, c):
    cl = closures(kind, d, K, c)
    return O.CallbackLoss(cl["f"], cl["grad_fx"], cl["hess_fx"], out_fn=cl["out_fn"], jac_yx=cl["jac_yx"],
                          grad_fy=cl["grad_fy"], hess_fy=cl["hess_fy"])


def callback_loss(losses, kind, d, K, c):
    cl = closures(kind, d, K, c)
    return losses.callback(cl["f"], cl["grad_fx"], cl["hess_fx"], out_fn=cl["out_fn"], jac_yx=cl["jac_yx"],
                           grad_fy=cl["grad_fy"], hess_fy=cl["hess_fy"])


def device_losses(losses, kind, K, c):
    """(f, out_fn) of the device kinds."""
    if kind == "softmax_ce":
        return losses.softmax_ce(K, c), losses.linear_softmax_ce(K, c)
    return losses.multi_least_squares(K, c), losses.linear_multi_ls(K, c)


def problem(N, d, K, soft=False):
    """A = randn(N, d)/√d, one-hot labels from argmax(A W + 0.3·noise) (default_rng(21)); x0 = 0.2·randn
    (default_rng(5)): not zero -- at x = 0 every P_ik = 1/K and a swapped k / l index goes unseen.
    soft: label-smoothed rows scaled by a per-sample weight in [0.5, 1.5], so s_i != 1."""
    rng = np.random.default_rng(21)
    A = rng.standard_normal((N, d)) / np.sqrt(d)
    W = rng.standard_normal((d, K))
    lab = np.argmax(A @ W + 0.3 * rng.standard_normal((N, K)), axis=1)
    Y = np.eye(K)[lab]
    if soft:
        Y = (0.9 * Y + 0.1 / K) * (0.5 + rng.random((N, 1)))
    x0 = 0.2 * np.random.default_rng(5).standard_normal(d * K)
    return A, Y, x0

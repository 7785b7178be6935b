"""NumPy restatement of the block eigensolver (csrc/mg_eig.hip, include/mghip_eig.h): LOBPCG with the pinned oracle's cycle
as preconditioner, built on pcg_reference.apply_A / apply_M.  It is the normative statement of the algorithm: what
tests/test_eig_cpu.py pins and tests/test_gpu_eig.py compares the device against.  Plain Python + NumPy.

Inner product: sum over interior cells (every vector has a zero ring).  Steps as numbered in the header."""
import numpy as np

import pcg_reference as R


def chol_orth_transform(G):
    """T = D^-1/2 L^-T with D = diag(G) and L L^T = D^-1/2 G D^-1/2; None where a pivot is non-positive or non-finite"""
    d = np.diag(G)
    if not (np.all(np.isfinite(G)) and np.all(d > 0)):
        return None
    s = 1.0 / np.sqrt(d)
    try:
        L = np.linalg.cholesky(G * np.outer(s, s))
    except np.linalg.LinAlgError:
        return None
    return s[:, None] * np.linalg.inv(L).T


def ritz(GA, GB, m):
    """step 5: lowest m pairs of G_A c = lambda G_B c -> (lambda[m], C[n, m]) or None when G_B is not positive definite"""
    GA, GB = 0.5 * (GA + GA.T), 0.5 * (GB + GB.T)
    if not np.all(np.isfinite(GB)):
        return None
    try:
        L = np.linalg.cholesky(GB)
    except np.linalg.LinAlgError:
        return None
    Li = np.linalg.inv(L)
    M = Li @ GA @ Li.T
    w, V = np.linalg.eigh(0.5 * (M + M.T))
    return w[:m], Li.T @ V[:, :m]


def gram(U, V):
    """G[a, b] = sum over cells of U_a V_b for blocks of shape (k, nx, ny)"""
    return np.einsum("aij,bij->ab", U, V)


def mix(S, C):
    """sum_a C[a, b] S_a"""
    return np.einsum("ab,aij->bij", C, S)


def default_start(m, nx, ny, seed=0):
    return np.random.default_rng(seed).standard_normal((m, nx, ny))


def exact_dirichlet(nx, ny, domain, count):
    """the `count` lowest eigenvalues of -Laplace_h with their (p, q) indices, ascending"""
    hx, hy = (domain[1] - domain[0]) / (nx - 1), (domain[3] - domain[2]) / (ny - 1)
    p, q = np.arange(1, nx - 1)[:, None], np.arange(1, ny - 1)[None, :]
    lam = 4 / hx**2 * np.sin(p * np.pi / (2 * (nx - 1)))**2 + 4 / hy**2 * np.sin(q * np.pi / (2 * (ny - 1)))**2
    order = np.argsort(lam, axis=None, kind="stable")[:count]
    return lam.ravel()[order], [(int(i // (ny - 2)) + 1, int(i % (ny - 2)) + 1) for i in order]


def exact_vector(nx, ny, p, q):
    i, j = np.arange(nx)[:, None], np.arange(ny)[None, :]
    return R.zero_ring(np.sin(p * np.pi * i / (nx - 1)) * np.sin(q * np.pi * j / (ny - 1)))


def lobpcg(mgo, x0, nev, tol=1e-8, max_iterations=100, pm=None, num_cycles=1):
    """-> (eigenvalues[nev], vectors[nev, nx, ny], info); mgo is a pcg_reference.make_oracle() hierarchy, x0 (m, nx, ny)"""
    hx, hy = mgo.h[0]
    m = x0.shape[0]
    A = lambda U: np.stack([R.apply_A(mgo, u) for u in U])
    X = np.stack([R.zero_ring(np.asarray(x, dtype=np.float64)) for x in x0])
    T = chol_orth_transform(gram(X, X))
    if T is None:
        raise ValueError("the start vectors are linearly dependent")
    X = mix(X, T)
    AX = A(X)
    G = gram(X, AX)
    lam, V = np.linalg.eigh(0.5 * (G + G.T))
    X, AX = mix(X, V), mix(AX, V)
    P = AP = None
    hist, status, converged, restarts, in_a_row, it = [], "max_iterations", False, 0, 0, 0
    rel = np.zeros(m)
    while True:
        Rm = AX - lam[:, None, None] * X                                           # 1
        rel = np.sqrt(np.einsum("aij,aij->a", Rm, Rm)) / lam
        hist.append(float(np.max(rel[:nev])))
        if hist[-1] < tol:
            status, converged = "converged", True
            break
        if it >= max_iterations:
            break
        W = np.stack([R.apply_M(mgo, r, pm, num_cycles) for r in Rm])              # 2
        C, WW = gram(X, W), gram(W, W)                                             # 3
        T = chol_orth_transform(0.5 * (WW + WW.T) - C.T @ C)
        if T is None:
            status = "breakdown"
            break
        W = mix(np.concatenate([X, W]), np.concatenate([-C @ T, T]))
        AW = A(W)
        dropped, result = False, None
        for _ in range(2):                                                         # 4, 5
            use_p = P is not None and not dropped
            S, AS = ([X, W, P], [AX, AW, AP]) if use_p else ([X, W], [AX, AW])
            S, AS = np.concatenate(S), np.concatenate(AS)
            GB, GA = gram(S, S), gram(S, AS)
            GB, GA = 0.5 * (GB + GB.T), 0.5 * (GA + GA.T)
            J = np.eye(S.shape[0])
            if use_p:
                Tp = chol_orth_transform(GB[2 * m:, 2 * m:])
                if Tp is None:
                    dropped = True
                    continue
                J[2 * m:, 2 * m:] = Tp
                GB, GA = J.T @ GB @ J, J.T @ GA @ J
            result = ritz(GA, GB, m)
            if result is None:
                if use_p:
                    dropped = True
                    continue
                break
            result = (result[0], J @ result[1], S, AS)
            break
        if dropped:
            restarts, in_a_row = restarts + 1, in_a_row + 1
        else:
            in_a_row = 0
        if result is None or in_a_row >= 2:
            status = "breakdown"
            break
        lam, Cf, S, AS = result
        P, AP = mix(S[m:], Cf[m:]), mix(AS[m:], Cf[m:])                            # 6
        X, AX = mix(X, Cf[:m]) + P, mix(AX, Cf[:m]) + AP
        it += 1
    vectors = X[:nev] / np.sqrt(hx * hy)
    return lam[:nev].copy(), vectors, {"iterations": it, "converged": converged, "status": status, "residuals": rel[:nev].copy(),
                                       "residual_history": hist, "restarts": restarts, "block_eigenvalues": lam.copy()}


# ---- the cases tests/test_eig_cpu.py pins and tests/test_gpu_eig.py runs on the device -------------------------------------
def jump_coefficient(nx, ny):
    """a = 10 for x < 1/2, else 1"""
    x = np.linspace(0.0, 1.0, nx)
    return np.where(x[:, None] < 0.5, 10.0, 1.0) * np.ones((nx, ny))


# name -> shape, domain, block size m, wanted pairs k, V(pre, post), smoother, coefficient, preconditioner precision
CASES = {
    "A": dict(nx=33, ny=65, domain=(0.0, 1.0, 0.0, 1.5), m=6, k=4, pre=1, post=1, smoother="jacobi", a=None, precision="double"),
    "A32": dict(nx=33, ny=65, domain=(0.0, 1.0, 0.0, 1.5), m=6, k=4, pre=1, post=1, smoother="jacobi", a=None, precision="single_managed"),
    "B": dict(nx=33, ny=33, domain=(0.0, 1.0, 0.0, 1.0), m=6, k=4, pre=2, post=2, smoother="jacobi", a=None, precision="double"),
    "C": dict(nx=65, ny=65, domain=(0.0, 1.0, 0.0, 1.0), m=8, k=6, pre=1, post=1, smoother="rbgs", a=None, precision="double"),
    "D": dict(nx=33, ny=33, domain=(0.0, 1.0, 0.0, 1.0), m=6, k=4, pre=2, post=2, smoother="jacobi", a="jump", precision="double"),
}
# iterations of the restatement at tol 1e-8 (0 restarts everywhere)
PINNED_ITERATIONS = {"A": 18, "A32": 18, "B": 16, "C": 16, "D": 15}
TOL = 1e-8


def case_oracle(name, oracle_classes=None):
    """oracle_classes: as pcg_reference.make_oracle's (None: the pinned pair)"""
    c = CASES[name]
    a = jump_coefficient(c["nx"], c["ny"]) if c["a"] == "jump" else None
    return R.make_oracle(c["nx"], c["ny"], a=a, pre=c["pre"], post=c["post"], smoother=c["smoother"],
                         omega=0.8 if c["smoother"] == "jacobi" else 1.0, domain=c["domain"], oracle_classes=oracle_classes)


def case_exact(name):
    """the k lowest eigenvalues: analytic for constant coefficients, numpy.linalg.eigvalsh of the assembled matrix otherwise"""
    c = CASES[name]
    if c["a"] is None:
        return exact_dirichlet(c["nx"], c["ny"], c["domain"], c["k"])[0]
    mgo = case_oracle(name)
    nx, ny = c["nx"], c["ny"]
    n = (nx - 2) * (ny - 2)
    M = np.empty((n, n))
    e = np.zeros((nx, ny))
    for col in range(n):
        i, j = 1 + col // (ny - 2), 1 + col % (ny - 2)
        e[i, j] = 1.0
        M[:, col] = R.apply_A(mgo, e)[1:-1, 1:-1].ravel()
        e[i, j] = 0.0
    return np.linalg.eigvalsh(0.5 * (M + M.T))[:c["k"]]


_RUNS = {}


def run_case(name, tol=TOL, max_iterations=100, oracle_classes=None):
    """the restatement on a case from the default start, computed once per process"""
    key = (name, tol, max_iterations, oracle_classes)
    if key not in _RUNS:
        c = CASES[name]
        _RUNS[key] = lobpcg(case_oracle(name, oracle_classes), default_start(c["m"], c["nx"], c["ny"]), c["k"], tol=tol,
                            max_iterations=max_iterations, pm=R.precision_manager(c["precision"]))
    return _RUNS[key]

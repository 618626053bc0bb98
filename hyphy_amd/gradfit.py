"""Positive model parameters by a limited-memory quasi-Newton iteration on the exact gradient.

The iteration works in theta = log x and maximises ``evaluate(x) -> logL``.  ``gradient(x)`` returns d log L / d x, or, with ``jac``,
d log L / d coefficients ([B, K], what ``HipPartition.branch_gradient_built`` answers) while ``jac(x)`` returns d coefficients / d x
([B, K, n]): the chain to a parameter is then a K-term dot product per branch.  Both are plain functions of the parameter vector: a
numpy model can drive the iteration as well as a partition on the device (``partition_callables``)."""
import numpy as np

MAX_STEP = float(np.log(4.0))      # no parameter changes by more than a factor of 4 in one iteration
MAX_HALVINGS = 40
ARMIJO = 1e-4


def _direction(g, pairs):
    """The L-BFGS two-loop recursion for ascent: H g with H from the stored (s, y = -(change of g)) pairs."""
    q, alphas = g.copy(), []
    for s, y in reversed(pairs):
        a = float(s @ q) / float(y @ s)
        alphas.append(a)
        q -= a * y
    if pairs:
        s, y = pairs[-1]
        q *= float(y @ s) / float(y @ y)
    for (s, y), a in zip(pairs, reversed(alphas)):
        q += (a - float(y @ q) / float(y @ s)) * s
    return q


def fit_parameters(evaluate, gradient, x0, jac=None, max_iter=200, tol=1e-6, memory=8):
    """Maximise ``evaluate`` over x > 0 from ``x0``.  Per iteration the L-BFGS direction in theta (steepest ascent while no curvature
    pair is stored or when the direction is not uphill), capped at MAX_STEP per parameter, halved until log L rises by ARMIJO times
    the predicted gain.  Stops when max |d log L / d theta| <= tol max(1, |log L|), when no halving gives a rise, or after
    ``max_iter`` iterations.  Returns (x, logL, iterations, history, largest |d log L / d theta| at the end)."""
    x = np.array(x0, dtype=np.float64).reshape(-1)
    if not np.all(x > 0):
        raise ValueError("parameters must be positive")

    def grad_theta(x):
        g = np.asarray(gradient(x), dtype=np.float64)
        if jac is not None:
            g = np.einsum("bk,bkn->n", g, np.asarray(jac(x), dtype=np.float64))
        return g.reshape(-1) * x

    theta, ll = np.log(x), float(evaluate(x))
    history, pairs, it = [ll], [], 0
    g = grad_theta(x)
    while it < max_iter and np.max(np.abs(g)) > tol * max(1.0, abs(ll)):
        it += 1
        d = _direction(g, pairs)
        if not d @ g > 0:
            d, pairs = g.copy(), []
        big = np.max(np.abs(d))
        if big > MAX_STEP:
            d *= MAX_STEP / big
        accepted = False
        for _ in range(MAX_HALVINGS):
            x_new = np.exp(theta + d)
            ll_new = float(evaluate(x_new))
            if ll_new >= ll + ARMIJO * float(d @ g):
                accepted = True
                break
            d *= 0.5
        if not accepted:
            break
        g_new = grad_theta(x_new)
        s, y = d, g - g_new
        if float(y @ s) > 1e-12 * float(np.linalg.norm(y) * np.linalg.norm(s)):
            pairs = (pairs + [(s.copy(), y.copy())])[-memory:]
        theta, x, ll, g = theta + d, x_new, ll_new, g_new
        history.append(ll)
    return x, ll, it, history, float(np.max(np.abs(g)))


def partition_callables(part, templates, coeffs_of, root_freqs):
    """(evaluate, gradient) over a one-class ``HipPartition`` for a template model: ``coeffs_of(x)`` gives the coefficient rows [B, K]
    over ``templates`` [K, D, D] (for example x_b = (t_b, omega t_b) with a global omega).  ``evaluate`` is a full pass over matrices
    built on the device; ``gradient`` is ``branch_gradient_built`` over all branches, d log L / d coefficients [B, K], behind a full
    pass at ``x`` when the last one was made elsewhere.  Pass the Jacobian of ``coeffs_of`` to ``fit_parameters`` as ``jac``."""
    B = int(part.B)
    nodes = np.arange(B, dtype=np.int64)
    part.set_q_templates(np.asarray(templates, dtype=np.float64))
    last = {"x": None}

    def evaluate(x):
        last["x"] = np.array(x, dtype=np.float64)
        part.build_q(np.ascontiguousarray(coeffs_of(x), dtype=np.float64))
        return part.evaluate_built(nodes, nodes, root_freqs)

    def gradient(x):
        if last["x"] is None or not np.array_equal(last["x"], np.asarray(x, dtype=np.float64)):
            evaluate(x)
        return part.branch_gradient_built(nodes, np.ascontiguousarray(coeffs_of(x), dtype=np.float64))[0]

    return evaluate, gradient

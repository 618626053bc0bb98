"""Branch lengths by a safeguarded diagonal Newton iteration over all branches at once.

The iteration works in theta_b = log t_b.  ``derivatives(t)`` returns, per branch, the first and second derivative (d1, d2) of log L
in a multiplier on the branch's rate matrix at 1 — what ``HipPartition.branch_derivatives`` answers for G = Q_b — so that in theta
the first derivative is d1 and the second d2 + d1.  Both callables are plain functions of the vector of branch lengths: a numpy model
can drive the iteration as well as a partition on the device (``partition_callables``)."""
import numpy as np

MAX_STEP = float(np.log(4.0))      # no branch length changes by more than a factor of 4 in one iteration
MAX_HALVINGS = 40


def fit_branch_lengths(evaluate, derivatives, t0, max_iter=50, tol=1e-8):
    """Maximise ``evaluate(t) -> logL`` over the branch lengths t > 0 from ``t0``.  Per iteration and branch the Newton step in
    theta = log t, -d1 / (d2 + d1), where the curvature d2 + d1 is negative, otherwise a step of MAX_STEP uphill; every step is
    capped at MAX_STEP, and the whole step is halved until log L does not fall.  Stops when max_b |d1_b| <= tol max(1, |log L|),
    when no halving of the step keeps log L from falling, or after ``max_iter`` iterations.
    Returns (t, logL, iterations, history): ``history`` holds log L at ``t0`` and after every accepted step."""
    t = np.array(t0, dtype=np.float64).reshape(-1)
    if not np.all(t > 0):
        raise ValueError("branch lengths must be positive")
    theta = np.log(t)
    ll = float(evaluate(t))
    history = [ll]
    it = 0
    while it < max_iter:
        d1, d2 = (np.asarray(x, dtype=np.float64) for x in derivatives(t))
        if not np.max(np.abs(d1)) > tol * max(1.0, abs(ll)):
            break
        it += 1
        h = d2 + d1
        with np.errstate(divide="ignore", invalid="ignore"):
            step = np.where(h < 0, -d1 / np.where(h < 0, h, -1.0), np.sign(d1) * MAX_STEP)
        step = np.clip(step, -MAX_STEP, MAX_STEP)
        accepted = False
        for _ in range(MAX_HALVINGS):
            t_new = np.exp(theta + step)
            ll_new = float(evaluate(t_new))
            if ll_new >= ll:
                accepted = True
                break
            step = step * 0.5
        if not accepted:
            break
        theta, t, ll = theta + step, t_new, ll_new
        history.append(ll)
    return t, ll, it, history


def partition_callables(part, unit_Q, root_freqs, rates=None, weights=None):
    """(evaluate, derivatives) over a ``HipPartition``: branch b of class c runs under Q = rates[c] t_b unit_Q[b] (``unit_Q``:
    [B, D, D] rate matrices of unit length; ``rates`` and ``weights``: [C], needed when the partition has more than one class).
    ``evaluate`` is a full pass (``evaluate`` / ``evaluate_categories``); ``derivatives`` calls ``branch_derivatives`` with G = Q,
    behind a full pass at ``t`` when the last one was made elsewhere."""
    unit_Q = np.asarray(unit_Q, dtype=np.float64)
    B = unit_Q.shape[0]
    nodes = np.arange(B, dtype=np.int64)
    C = int(part.C)
    if C > 1 and (rates is None or weights is None):
        raise ValueError("rates and weights are needed for a partition with rate classes")
    rates = np.ones(1) if rates is None else np.asarray(rates, dtype=np.float64)
    if rates.shape != (C,):
        raise ValueError(f"expected {C} rates, got {rates.shape}")
    last = {"t": None}

    def scaled(t):
        return rates[:, None, None, None] * np.asarray(t, dtype=np.float64)[None, :, None, None] * unit_Q[None]   # [C, B, D, D]

    def evaluate(t):
        q = scaled(t)
        last["t"] = np.array(t, dtype=np.float64)
        if C == 1:
            return part.evaluate(nodes, nodes, q[0], root_freqs)
        return part.evaluate_categories(nodes, nodes, q, weights, root_freqs)

    def derivatives(t):
        if last["t"] is None or not np.array_equal(last["t"], np.asarray(t, dtype=np.float64)):
            evaluate(t)
        d1, d2, _ = part.branch_derivatives(nodes, np.ascontiguousarray(scaled(t).transpose(1, 0, 2, 3)), weights)
        return d1, d2

    return evaluate, derivatives

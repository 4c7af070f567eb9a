"""Inputs and CPU references of the lsq_linear_act_quant_solve_half tests, shared by tests/test_linear_act_solve_host.py (a
numpy model of the kernel's arithmetic against the exact oracle) and tests/test_gpu_linear_act_solve.py (the kernel):
deterministic bf16 / fp16 rows, the clamp bounds rounded into the type, the oracle's v1 per case (computed once), and the
model -- counts per distinct key, prefix sums in key order, the run-wise candidate test, the cost without sum a^2 and the
(cost, position) argmin."""

import functools

import numpy as np
import torch

import detgen
from oracle import lsq_exact

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
LS = (3, 5, 64, 65, 193, 800, 4104, 70001, 1, 2)      # li indexes this; the two short rows have n < 3 keys
BOUNDS = (-1, 2.0, 1.3, 0.5)      # none, one both types hold, one neither holds, one that clamps about two thirds of a row
SKIPS = (1, 3)
SCHEMES = ('ls-2', 'ls-T')


def n_rows(L: int) -> int:
    return 2 if L == 70001 else (3 if L < 3 else 7)


def rounded(alpha: float, dtype) -> float:
    """The bound as Tensor.clamp rounds it into a tensor of the type; negative: no clamp."""
    return torch.tensor(alpha, dtype=dtype).item() if alpha >= 0 else float(alpha)


@functools.lru_cache(maxsize=None)
def rows(li: int, dt: str) -> torch.Tensor:
    """x [n, L] of the type on the CPU; nothing writes into it."""
    L = LS[li]
    return detgen.normal(f'actsolvehalf.x.{li}', (n_rows(L), L), seed=li, scale=1.2).to(DTYPES[dt])


def clamped32(x: torch.Tensor, alpha: float) -> np.ndarray:
    """x (16-bit) converted to fp32 and clamped to a bound that is a value of its type: every element stays one."""
    xf = x.float()
    return (xf.clamp(-alpha, alpha) if alpha >= 0 else xf).numpy()


def cases():
    """(li, L, dt, bound, skip, scheme) over everything."""
    return [(li, L, dt, b, skip, scheme) for li, L in enumerate(LS) for dt in DTYPES for b in BOUNDS for skip in SKIPS
            for scheme in SCHEMES]


def oracle_rows(xc: np.ndarray, ternary: bool, skip: int):
    """(v1 [n] fp32, found [n] bool) of oracle.lsq_exact on rows that are already clamped fp32."""
    v1, found = [], []
    for r in xc:
        d = {}
        v1.append(lsq_exact.solve_row(r, ternary, skip, details=d))
        found.append(len(d['values']) > 0)
    return np.array(v1, dtype=np.float32), np.array(found)


@functools.lru_cache(maxsize=None)
def oracle(li: int, dt: str, bound: float, skip: int, scheme: str):
    """The oracle on case (li, dt, bound, skip, scheme): computed once, shared, left unchanged."""
    return oracle_rows(clamped32(rows(li, dt), rounded(bound, DTYPES[dt])), scheme == 'ls-T', skip)


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic
def _cost(v, below_cnt, below_sum, eq_cnt, n, total, ternary):
    """csrc/lsq_solver_math.h cost_of: the closed-form cost^2 minus the constant sum a^2."""
    dn = float(n)
    above_cnt = dn - below_cnt - eq_cnt
    above_sum = total - below_sum - eq_cnt * v
    dev = (v * below_cnt - below_sum) + (above_sum - v * above_cnt)
    quad = -2.0 * v * total + dn * v * v
    if ternary:
        return quad - 2.0 * v * dev + dn * v * v
    return quad - dev * dev / dn


def _hits(v, nxt, lo_cnt, lo_sum, n, total, ternary):
    """position_is_candidate, vectorised over positions: v <= m <= nxt for m2, and for m1 unless ternary."""
    with np.errstate(divide='ignore', invalid='ignore'):
        hi_mean = (total - lo_sum) / (n - lo_cnt)
        m2 = 0.5 * hi_mean
        hit = (v <= m2) & (m2 <= nxt)
        if not ternary:
            m1 = 0.5 * (lo_sum / lo_cnt + hi_mean)
            hit |= (v <= m1) & (m1 <= nxt)
    return hit


def model_row(row: np.ndarray, ternary: bool, skip: int):
    """(v1 fp32, found) the way the kernel computes them from a clamped fp32 row whose values are values of a 16-bit type:
    a table of one count per distinct magnitude (= per key, in key order), a key's sum as count x value, exclusive prefix
    counts and fp64 prefix sums in key order, each key a run of equal values tested at its interior positions and at its
    last position against the next key's value, the cost without sum a^2, the minimum by (cost, first position of the run);
    the ternary extra candidate comes last."""
    a = np.abs(np.asarray(row, dtype=np.float32).reshape(-1)[::skip])
    n = a.size
    vals, cnts = np.unique(a, return_counts=True)
    v = vals.astype(np.float64)
    c = cnts.astype(np.float64)
    s = c * v                                          # exact: count < 2^31, at most 11 significant bits in the value
    p_incl = np.cumsum(s)
    total = float(p_incl[-1])
    p0 = p_incl - s
    r0 = np.cumsum(cnts) - cnts
    succ = np.append(v[1:], np.inf)
    best = (np.inf, 1 << 62, np.float32(0.0))
    if n >= 3:
        # every sorted position i of the row at once: run q, t = its place in the run; the sum up to and including i is
        # p0 + (t + 1) v (the kernel's expression); the successor is v inside a run, the next key's value at its end
        q = np.repeat(np.arange(v.size), cnts)
        pos = np.arange(n)
        t = pos - r0[q]
        nxt = np.where(t == cnts[q] - 1, succ[q], v[q])
        hit = _hits(v[q], nxt, pos + 1.0, p0[q] + (t + 1.0) * v[q], float(n), total, ternary) & (pos >= 1) & (pos <= n - 2)
        runs = np.unique(q[hit])
        if runs.size:
            costs = _cost(v[runs], r0[runs].astype(np.float64), p0[runs], c[runs], n, total, ternary)
            i = np.lexsort((r0[runs], costs))[0]
            best = (float(costs[i]), int(r0[runs[i]]), np.float32(v[runs[i]]))
    if ternary and n > 0:
        mean = total / n
        if v[0] > 0.5 * mean:
            half = np.float32(float(np.float32(mean)) / 2)
            cand = (_cost(float(half), 0.0, 0.0, 0.0, n, total, True), n + 1, half)
            if cand[:2] < best[:2]:
                best = cand
    return best[2], best[1] != 1 << 62


def model_rows(xc: np.ndarray, ternary: bool, skip: int):
    out = [model_row(r, ternary, skip) for r in xc]
    return np.array([o[0] for o in out], dtype=np.float32), np.array([o[1] for o in out])

"""Inputs of the rollout kernel tests (tests/test_rollout_ref_host.py, tests/test_gpu_rollout_kernels.py), built once in
numpy with a fixed seed so that the host tests judge -- margins, negative controls -- exactly what the GPU tests launch.

Common to all cases: hist_y is a per-series random walk with increments ~0.02 around a different level per series, hist_e1 and
hist_e2 are its fp64 EMAs rounded to fp32, the taps are the fp32 EWMA weights.  Every array has the dtype the kernel reads."""
import numpy as np

import rollout_ref as rr

J = 1e-4                    # the jitter of the failure matrix; its rows are written in multiples of it
DX = 1.0 / 252
BOUND = 2e-4                # |out - fp64| <= BOUND * max(1, max |fp64 path|): the project's bound for this comparison
ENGINE_BOUND = 5e-5         # re-substitution vs the default engine, of the paths' magnitude

# (delta = rho - acc0 in J, [1/2 dx v^2 per step in J; the last value repeats], expected info,
#  {step: rung} with rung 0 / 1 / 2 = jitter, 10 jitter, 100 jitter and 3 = exhausted,
#  {step: pvar / J} and {step: d2 / J} at the designed steps)
FAILURE_ROWS = [
    (4, [8, 5], 0, {}, {0: 4}, {0: 12}),
    (4, [3.5, 5], 0, {0: 0}, {0: -0.5}, {0: 3}),
    (4, [2.5, 5], 0, {0: 1}, {0: -1.5}, {0: 1}),
    (30, [18, 5], 0, {0: 2}, {0: -12}, {0: 6}),
    (300, [160, 5], -1, {0: 3}, {0: -140}, {0: 20}),
    (4, [1, 10, 5], 1, {0: 1}, {0: -3, 1: 4, 2: 5}, {0: -2, 1: 14}),
    (4, [1, 5.5, 5], 1, {0: 1, 1: 0}, {0: -3, 1: -0.5}, {0: -2, 1: 5}),
    (150, [60, 1, 5], -2, {0: 2, 1: 3}, {0: -90, 1: -929}, {0: -30}),
    (300, [1, 5], -1, {0: 3}, {0: -299}, {0: -298}),
]
FAILURE_DELTAS = [4, 30, 150, 300]                    # series g carries the rows whose delta this is


def taps(k):
    """EWMA.py:21-24 in fp32: w_j ~ alpha (1 - alpha)^(k-1-j), normalised."""
    alpha = 2.0 / (k + 1)
    w = alpha * np.power(1.0 - alpha, np.arange(k - 1, -1, -1, dtype=np.float64))
    return (w / w.sum()).astype(np.float32)


def histories(rng, levels, k):
    """(hist_y, hist_e1, hist_e2 [G,k] fp32, ema_prev [G] fp32, w [k] fp32) for one random walk per level."""
    G = len(levels)
    w = taps(k)
    y = (np.asarray(levels, dtype=np.float64)[:, None] + np.cumsum(0.02 * rng.standard_normal((G, 3 * k)), axis=1)
         ).astype(np.float32)
    y, e1, e2 = rr.ema_tails(y, w, 2)
    # e1[t] is the EMA of the k values BEFORE t: the tails the kernel continues from end at the last train point
    f = lambda a: np.ascontiguousarray(a[:, -k:].astype(np.float32))
    return f(y), f(e1), f(e2), np.ascontiguousarray(e1[:, -1].astype(np.float32)), w


def _common(rng, levels, S, H, k, mode):
    G = len(levels)
    hy, e1, e2, ema_prev, w = histories(rng, levels, k)
    lv = np.asarray(levels, dtype=np.float64)
    inp = dict(hist_y=hy, hist_e1=e1, hist_e2=e2, ema_prev=ema_prev, w=w, k=k, mean_mode=mode, mr_theta=0.5,
               mr_latent=(lv + 0.1 * rng.standard_normal(G)).astype(np.float32),
               latent=(lv + 0.1 * rng.standard_normal(G) + 0.1).astype(np.float32),
               tau=0.05 * rng.standard_normal(G) + 0.03 * np.arange(1, G + 1),
               acc0=rng.uniform(0.5, 2.0, G),
               z=rng.standard_normal((G, S, H)).astype(np.float32))
    if mode == 4:                                          # a mean given at the H test points; hist_y is ignored, k = 1
        inp["hist_e1"] = (lv[:, None] + 0.01 * np.cumsum(rng.standard_normal((G, H)), axis=1)).astype(np.float32)
    return inp


def failure_inputs(S, H, mode, theta=None, jitter=J, seed=20240611, k=25):
    """The failure matrix: G = 4 series with delta in FAILURE_DELTAS, path s of a series walks the rows of that delta
    cyclically, every path with its own z; k beyond the LDS ring limit selects the wave-per-path engine.  Returns (inp, row [G,S]): inp holds bordered_ref's arguments by name."""
    rng = np.random.default_rng(seed)
    k = 1 if mode == 4 else k
    G = len(FAILURE_DELTAS)
    inp = _common(rng, [0.7, 1.5, 2.5, 4.0], S, H, k, mode)
    inp.update(theta=theta, jitter=jitter, dx=np.full(G, DX, dtype=np.float32))
    inp["rho"] = inp["acc0"] + np.asarray(FAILURE_DELTAS, dtype=np.float64) * J
    dx = float(np.float32(DX))
    row = np.zeros((G, S), dtype=np.int64)
    pv = np.zeros((G, S, H), dtype=np.float32)
    for g, delta in enumerate(FAILURE_DELTAS):
        mine = [i for i, r in enumerate(FAILURE_ROWS) if r[0] == delta]
        for s in range(S):
            row[g, s] = mine[s % len(mine)]
            m = FAILURE_ROWS[row[g, s]][1]
            mult = np.asarray([m[min(i, len(m) - 1)] for i in range(H)], dtype=np.float64)
            pv[g, s] = np.sqrt(2.0 * mult * J / dx)
    inp["pred_vol"] = pv
    return inp, row


HEALTHY_DX = [1.0 / 252, 1.0 / 52, 1.0 / 12]
HEALTHY_DELTA = [0.0, -0.3, 2 * J]           # the last: base = -2 J, its first pvar positive (dx = 1/12, vol >= 0.17: >= 12 J)


def healthy_inputs(S, H, k, mode, theta=None, seed=7, jitter=J):
    """Accuracy cases: G = 3 series, every per-series scalar different."""
    rng = np.random.default_rng(seed + 1000 * mode + 7 * S + 13 * H + 17 * k)
    G = 3
    inp = _common(rng, [0.7, 2.2, 4.5], S, H, 1 if mode == 4 else k, mode)
    inp.update(theta=theta, jitter=jitter, dx=np.asarray(HEALTHY_DX, dtype=np.float32))
    inp["rho"] = inp["acc0"] + np.asarray(HEALTHY_DELTA)
    inp["pred_vol"] = (0.17 + 0.15 * rng.random((G, S, H))).astype(np.float32)
    return inp


_REF_ARGS = ("rho", "tau", "acc0", "dx", "hist_y", "hist_e1", "hist_e2", "ema_prev", "mr_latent", "latent", "w", "pred_vol",
             "z", "k", "mean_mode", "theta", "mr_theta", "jitter")


def run_ref(inp, **kw):
    return rr.bordered_ref(*(inp[n] for n in _REF_ARGS), **kw)


def path_bound(ref, mask=None):
    """BOUND * max(1, max |ref path|) per path [G,S,1], over the compared steps."""
    a = np.abs(ref) if mask is None else np.where(mask, np.abs(ref), 0.0)
    return BOUND * np.maximum(1.0, a.max(axis=-1, keepdims=True))


def margins(trace, mask, jitter):
    """The distance of every comparison a compared step made from its decision, in units of J: min over pvar > 0, the
    rungs tried (pvar + jitter 10^r > 0) and d2 > 0.  Steps outside ``mask`` do not count."""
    pvar, d2 = trace["pvar"], trace["d2"]
    dist = np.minimum(np.abs(pvar), np.abs(d2))
    jit = float(np.float32(jitter))
    tried = ~(pvar > 0)
    for r in range(3):
        dist = np.where(tried, np.minimum(dist, np.abs(pvar + jit)), dist)
        tried = tried & ~(pvar + jit > 0)
        jit *= 10.0
    return float(np.where(mask, dist, np.inf).min() / J)


# (name, mean_mode, theta, S, H, k, engine): engine "lane" (scratch NULL, k inside the LDS ring), "wave" (scratch NULL, k beyond
# the ring: a wave per path, append-only), "resub" (scratch given: re-substitution)
HEALTHY_CASES = [
    ("m0_S1_H1_k1", 0, None, 1, 1, 1, "lane"),
    ("m0t_S5_H2_k2", 0, 0.5, 5, 2, 2, "lane"),
    ("m1_S64_H3_k25", 1, None, 64, 3, 25, "lane"),
    ("m1t_S65_H4_k64", 1, 0.3, 65, 4, 64, "lane"),
    ("m2_S130_H7_k65", 2, None, 130, 7, 65, "lane"),
    ("m2t_S5_H8_k25", 2, 0.5, 5, 8, 25, "lane"),
    ("m3_S64_H63_k25", 3, None, 64, 63, 25, "lane"),
    ("m3t_S65_H64_k2", 3, 0.5, 65, 64, 2, "lane"),
    ("m4_S5_H65", 4, None, 5, 65, 1, "lane"),
    ("m4t_S130_H100", 4, 0.5, 130, 100, 1, "lane"),
    ("m0t_S5_H256_k64", 0, 0.2, 5, 256, 64, "lane"),
    ("m3_S5_H257_k65", 3, None, 5, 257, 65, "lane"),
    ("m0_S5_H300_k25", 0, None, 5, 300, 25, "lane"),
    ("m0_S5_H4_k2048", 0, None, 5, 4, 2048, "wave"),
    ("m0_S5_H8_k581", 0, None, 5, 8, 581, "lane"),
    ("m0_S5_H8_k582", 0, None, 5, 8, 582, "wave"),
    ("m3t_S5_H8_k581", 3, 0.5, 5, 8, 581, "lane"),
    ("m3t_S5_H8_k582", 3, 0.5, 5, 8, 582, "wave"),
    ("m1_S5_H8_k295", 1, None, 5, 8, 295, "lane"),
    ("m1_S5_H8_k296", 1, None, 5, 8, 296, "wave"),
    ("m2_S5_H8_k197", 2, None, 5, 8, 197, "lane"),
    ("m2_S5_H8_k198", 2, None, 5, 8, 198, "wave"),
    ("r_m0t_S5_H256_k25", 0, 0.5, 5, 256, 25, "resub"),
    ("r_m3_S5_H257_k25", 3, None, 5, 257, 25, "resub"),
    ("r_m4t_S5_H300", 4, 0.5, 5, 300, 1, "resub"),
    ("r_m1_S9_H7_k25", 1, None, 9, 7, 25, "resub"),
]


def lane_ring_fits(mode, k):
    """csrc/rollout.hip: a lane per path when levels * k * 256 + 8 k <= 150 KB."""
    levels = {0: 1, 1: 2, 2: 3, 3: 1, 4: 0}[mode]
    return levels * k * 256 + 8 * k <= 150 * 1024


# volt_rollout_shared_f32 at G = 3: (mean_mode, S, H, k).  tewma at k = 1 stays at H = 2: its mean is then
# 3 y[t-1] - 3 y[t-2] + y[t-3], a recursion with a triple root at 1, which returns a rounding made at step s as
# (t - s + 1)(t - s + 2) / 2 times itself at step t.  The fp32 rounding of the stored samples alone -- which any implementation
# with fp32 outputs makes -- then lands 5.6 x the bound from the fp64 run at H = 300 (0.11 x at H = 65), measured on the
# restatement with sample_dtype = fp32.  A case is admitted when that figure is <= SHARED_CONDITION = 1/20: the kernel rounds up
# to four more values per step (the three levels' sums and the mean), and the bound is for its arithmetic, not for the input's
# amplification (test_rollout_ref_host.py::test_shared_cases_are_well_conditioned).
SHARED_CASES = [(0, 1, 1, 1), (0, 5, 300, 25), (1, 9, 2, 25), (1, 5, 65, 300), (2, 9, 65, 25), (2, 1, 2, 1), (2, 5, 300, 300),
                (2, 5, 2, 300), (3, 5, 65, 25), (3, 9, 300, 300), (3, 1, 1, 25), (0, 1, 300, 1), (1, 1, 65, 1)]
SHARED_CONDITION = 0.05
SHARED_LEVELS = [0.7, 2.2, 4.5]


def shared_inputs(mode, S, H, k):
    """(hist_y, hist_e1, hist_e2, ema_prev, mr_latent, w, e): shared_ref's leading arguments; e ~ N(0, 0.02^2)."""
    rng = np.random.default_rng(31 + mode + 3 * S + 5 * H + 7 * k)
    hy, e1, e2, ema_prev, w = histories(rng, SHARED_LEVELS, k)
    mrl = (np.asarray(SHARED_LEVELS) + 0.1 * rng.standard_normal(3)).astype(np.float32)
    e = (0.02 * rng.standard_normal((3, S, H))).astype(np.float32)
    return hy, e1, e2, ema_prev, mrl, w, e

#!/usr/bin/env python
"""A/B of the vol forecaster's posterior (models/BMGP.py: BMGP and MultitaskBMGP in eval mode) between two checkouts: same bits.

    python scripts/ab_vol_posterior.py --tree <checkout> --out digests.json     # SHA-256 of every result
    python scripts/ab_vol_posterior.py --compare a.json b.json                  # exit 1 unless every digest is equal

One process imports ONE volt_amd, so run it once per checkout (``--tree``: the checkout whose volt_amd is imported, default
this one; it must be built).  Per case the four routes -- solver="dense", and solver="linear" with posterior "solve", "sweep",
"chain" -- and of each posterior ``.mean``, ``.covariance_matrix``, ``.variance`` and one ``sample(torch.Size((3,)),
base_samples=...)`` with fixed base samples.  The cases are fixed and seeded on the host:
  BMGP           fp32 and fp64, one series (T = 1) and T in {3, 8, 65} series, N in {1, 3, 65, 399} (N = 1: the constructor
                 reads x[1], so what is hashed there is its IndexError), and 8 x 4096
  MultitaskBMGP  N in {1, 3, 65, 399} x T in {1, 3, 8, 64} (the Kronecker path takes T <= 64), and 4096 x 8
  test points    H in {1, 20, 65, 130} (H = 20 at N = 4096): ascending beyond the grid; from H = 20 also shuffled with two
                 points inside the grid and one on it, and ascending with a duplicate
  a failure      per model at 3 x 65, H = 20: a negative noise (series / direction 0), every route
An exception is a result: its type and message are hashed in place of the tensor (the failing cases; a factor of a singular
covariance that runs out of jitter).  NaNs are canonicalised before hashing; nothing else is: -0.0 is not 0.0.
Speed is scripts/bench_bm_posterior.py's subject, run on the two checkouts alternately (profiles/vol_posterior/ab.txt).
"""
import argparse
import hashlib
import json
import os
import sys
import warnings

import numpy as np

NS, HS = (1, 3, 65, 399), (1, 20, 65, 130)
ROUTES = (("dense", "solve"), ("linear", "solve"), ("linear", "sweep"), ("linear", "chain"))
RAISED = {}                                   # exception type -> results it stood for (reported beside the digests)


def digest(t):
    a = t.detach().cpu().contiguous().numpy()
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), np.array(np.nan, dtype=a.dtype), a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


def rng(name):
    return np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little"))


def grid(r, N):
    return np.cumsum(r.uniform(0.5, 1.5, N)) / 252.0


def test_points(r, x, H):
    """{order: xs [H]}: "asc" beyond the grid; "shuffled" with two points inside the grid and one on it; "dup" with a twin."""
    beyond = x[-1] + np.cumsum(r.uniform(0.5, 1.5, H)) / 252.0
    out = {"asc": beyond}
    if H >= 20:
        mixed = beyond.copy()
        mixed[:3] = [0.37 * x[-1], 0.81 * x[-1], x[len(x) // 2]]
        out["shuffled"] = r.permutation(mixed)
        dup = beyond.copy()
        dup[7] = dup[6]
        out["dup"] = dup
    return out


def hash_posterior(torch, out, name, build, xs, r):
    """Every result of one posterior call under ``name``; an exception stands for the results it kept from being computed."""
    def put(key, fn):
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out[f"{name}/{key}"] = digest(fn())
        except Exception as e:                                            # noqa: BLE001 -- the exception IS the result
            out[f"{name}/{key}"] = hashlib.sha256(f"{type(e).__name__}: {e}".encode()).hexdigest()
            RAISED[type(e).__name__] = RAISED.get(type(e).__name__, 0) + 1
            return e
    post = []
    if put("call", lambda: (post.append(build()(xs)), torch.zeros(0))[1]) is not None:
        return
    post = post[0]
    z = torch.as_tensor(r.standard_normal((3,) + tuple(post.mean.shape))).to(post.mean.dtype).to(xs.device)
    put("mean", lambda: post.mean)
    put("covariance_matrix", lambda: post.covariance_matrix)
    put("variance", lambda: post.variance)
    put("sample", lambda: post.sample(torch.Size((3,)), base_samples=z))
    torch.cuda.synchronize()


def digest_cases(torch, dev):
    from volt_amd import gp, ops
    from volt_amd.models import BMGP, MultitaskBMGP
    out = {}
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)

    class NegativeNoise(gp.GaussianLikelihood):                           # series 0: a negative noise, the others as they are
        @property
        def noise(self):
            n = gp.GaussianLikelihood.noise.fget(self).clone()
            n.reshape(-1)[0] = -1.0
            return n

    def bmgp(x, y, dt, solver, posterior, fail=False):
        bs = torch.Size(y.shape[:-1])
        lh = (NegativeNoise if fail else gp.GaussianLikelihood)(batch_shape=bs).to(dev).to(dt)
        m = BMGP(t(x, dt), t(y, dt), lh, solver=solver, posterior=posterior).to(dev).to(dt)
        with torch.no_grad():
            if len(bs):
                m.covar_module.raw_vol.copy_(torch.linspace(-1.5, 0.5, bs[0], dtype=dt).reshape(-1, 1))
                lh.raw_noise.copy_(torch.linspace(-3.0, 0.0, bs[0], dtype=dt).reshape(-1, 1))
            else:
                m.covar_module.raw_vol.fill_(-0.7)
                lh.raw_noise.fill_(-2.0)
        return m.eval()

    def multitask(x, Y, p, solver, posterior):
        T = Y.shape[1]
        lh = gp.MultitaskGaussianLikelihood(num_tasks=T).to(dev)
        m = MultitaskBMGP(t(x, torch.float32), t(Y, torch.float32), lh, solver=solver, posterior=posterior).to(dev)
        task, data = m.covar_module.task_covar_module, m.covar_module.data_covar_module
        with torch.no_grad():
            for prm, v in zip((data.raw_vol, task.covar_factor, task.raw_var, lh.raw_task_noises, lh.raw_noise), p):
                prm.copy_(t(v, torch.float32).reshape(prm.shape))
        return m.eval()

    def mt_params(r, T):
        return (r.standard_normal(1) * 0.5 - 1.0, r.standard_normal((T, 1)) * 0.5, r.standard_normal(T) - 1.0,
                r.standard_normal(T) - 3.0, r.standard_normal(1) - 4.0)

    def routes(name, x, dt, H_list, build, fail=False):
        print(name, file=sys.stderr, flush=True)
        for H in H_list:
            for order, xs in test_points(rng(f"xs/{name}/{H}"), x, H).items():
                for solver, posterior in ROUTES:
                    tag = f"{name}/H{H}/{order}/{solver}-{posterior}"
                    hash_posterior(torch, out, tag, lambda: build(solver, posterior), t(xs, dt), rng("z/" + tag))
                if fail:
                    break

    for dt, dn in ((torch.float32, "f32"), (torch.float64, "f64")):
        for T, N in [(T, N) for N in NS for T in (1, 3, 8, 65)] + [(8, 4096)]:
            for fail in ((False, True) if (T, N) == (3, 65) else (False,)):
                name = f"bmgp/{dn}/{T}x{N}" + ("/fail" if fail else "")
                r = rng(name)
                x = grid(r, N)
                y = np.cumsum(r.standard_normal((T, N)) * 0.05, axis=1) - 2.0
                y = y[0] if T == 1 else y
                routes(name, x, dt, [20] if fail or N > 399 else HS,
                       lambda solver, posterior: bmgp(x, y, dt, solver, posterior, fail), fail)

    real_prologue = ops.kron_prologue
    for N, T in [(N, T) for N in NS for T in (1, 3, 8, 64)] + [(4096, 8)]:
        for fail in ((False, True) if (N, T) == (65, 3) else (False,)):
            name = f"multitask/{N}x{T}" + ("/fail" if fail else "")
            r = rng(name)
            x = grid(r, N)
            Y = -1.5 + np.cumsum(r.standard_normal((N, 1)), 0) * 0.05 + np.cumsum(r.standard_normal((N, T)), 0) * 0.03
            p = mt_params(r, T)
            if fail:                                                      # direction 0: a negative sigma_0^2 behind the prologue
                def negated(params, xg, Yg, ws, *a, **kw):
                    res = real_prologue(params, xg, Yg, ws, *a, **kw)
                    ws.sigma2[:1].neg_()
                    return res
                ops.kron_prologue = negated
            try:
                routes(name, x, torch.float32, [20] if fail or N > 399 else HS,
                       lambda solver, posterior: multitask(x, Y, p, solver, posterior), fail)
            finally:
                ops.kron_prologue = real_prologue
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", help="write the digests to this JSON file")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        A, B = (json.load(open(f)) for f in a.compare)
        bad = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
        print(f"{len(A)} and {len(B)} digests, {len(bad)} differ")
        for k in bad:
            print("  ", k, A.get(k), B.get(k))
        sys.exit(1 if bad or not A else 0)
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    d = digest_cases(torch, torch.device("cuda"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(d, fh, indent=0, sort_keys=True)
    print(json.dumps({"tree": os.path.abspath(a.tree), "digests": len(d), "results_that_are_exceptions": RAISED,
                      "all": hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()

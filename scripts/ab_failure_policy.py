#!/usr/bin/env python
"""A/B of the failure policy (volt_amd/safe.py: the jitter ladder, the NaN look, the internal-error fall-back) between two
checkouts: same outputs, same warnings, same exceptions, same calls of the library.

    python scripts/ab_failure_policy.py --tree <checkout> --out digests.json     # SHA-256 of every case
    python scripts/ab_failure_policy.py --compare a.json b.json                  # exit 1 unless every digest is equal

One process imports ONE volt_amd, so run it once per checkout (``--tree``: the checkout whose volt_amd is imported, default this
one; it must be built).  The cases are the rung table of tests/test_gpu_safe_ladder.py -- one pivot at -c with c = 0.3 s, 3 s,
30 s, 1 for first rung s (gpytorch's default per dtype, and a given 1e-4), the clean input, one NaN -- through every route:
  _safe_factor / psd_safe_cholesky   A = I with A[k,k] = -c, N in {8, 130}, batch 1 and 3, fp32 and fp64; and a half-precision A,
                                     which starts at the fp64 rung
  ExactMarginalLogLikelihood         the same A as K + sigma^2 I at the noise floor; the value and d / d raw_noise
  _safe_forms, _safe_draw            three grids / one crafted chain with a step of -c
  _chol_1x1                          the 1x1 predictive covariance at -c
Per case ONE digest of: the outputs' bytes, the jitter used, every warning (category, text), the exception (type, text) and the
(jitter, tables) of every call of the ops entry the route stands on.  NaNs are canonicalised before hashing; nothing else is.
The internal-error fall-back needs a trampled workspace and stays with tests/test_gpu_contract.py.
"""
import argparse
import hashlib
import inspect
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DENSE = ((8, 5), (130, 129))
RAISED = {}                                   # exception type -> cases that ended in it (reported beside the digests)


def digest(t):
    a = t.detach().cpu().contiguous().numpy() if hasattr(t, "detach") else np.asarray(t)
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), np.array(np.nan, dtype=a.dtype), a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


def table(s):
    return (("clean", None), ("rung0", 0.3 * s), ("rung1", 3 * s), ("rung2", 30 * s), ("exhausted", 1.0))


def digest_cases(torch, dev):
    from volt_amd import gp, ops, rollout_utils
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import vk_chain_ref as vk
    out, F32, F64 = {}, torch.float32, torch.float64
    firsts = ((F32, None, "f32-default"), (F64, None, "f64-default"), (F32, 1e-4, "f32-1e-4"), (F64, 1e-4, "f64-1e-4"))

    def case(name, entry, fn):
        """fn() -> the tensors and numbers to hash, run with ops.<entry> counted."""
        calls, real = [], getattr(ops, entry) if entry else None
        if entry:
            sig = inspect.signature(real)

            def counted(*a, **kw):
                b = sig.bind(*a, **kw)
                b.apply_defaults()
                calls.append((float(b.arguments["jitter"]), b.arguments.get("tables")))
                return real(*a, **kw)
            setattr(ops, entry, counted)
        try:
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                try:
                    res = [digest(r) if hasattr(r, "shape") else repr(r) for r in fn()]
                except Exception as e:                                        # noqa: BLE001 -- the exception IS the result
                    res = [f"{type(e).__name__}: {e}"]
                    RAISED[type(e).__name__] = RAISED.get(type(e).__name__, 0) + 1
        finally:
            if entry:
                setattr(ops, entry, real)
        torch.cuda.synchronize()
        what = {"result": res, "warnings": [(w.category.__name__, str(w.message)) for w in rec], "calls": calls}
        out[name] = hashlib.sha256(json.dumps(what, sort_keys=True).encode()).hexdigest()

    def dense(N, k, c, B, dt):
        A = torch.eye(N, dtype=dt, device=dev).repeat(B, 1, 1)
        if c is not None:
            A[B // 2, k, k] = -c
        return A

    def with_nan(A, idx):
        A = A.clone()
        A[idx] = float("nan")
        return A

    def factor(A, given):
        f, used = gp._safe_factor(A, given)
        return f.L, f.info, used

    V, _, r = vk.mixed_case(130, 70, 0)
    keep = [b for b in range(12) if (np.diff(V[b], prepend=0.0) > 0).all()][:3]
    H, S = 65, 9
    z64 = torch.tensor(np.random.default_rng(3).standard_normal((1, S, H)))
    for dt, given, tag in firsts:
        s = given if given is not None else (1e-6 if dt == F32 else 1e-8)
        print(tag, file=sys.stderr, flush=True)
        # ---- ops.potrf, ops.mll_step
        lh = gp.GaussianLikelihood().to(dev).to(dt)
        lh.noise_covar.raw_noise.data.fill_(-30.0)
        mll = gp.ExactMarginalLogLikelihood(lh, None)

        def mll_value(A, B, N):
            zeros = torch.zeros((B, N) if B > 1 else (N,), dtype=dt, device=dev)
            floor = lh.noise.detach().to(dt).reshape(()) * torch.eye(N, dtype=dt, device=dev)
            lh.noise_covar.raw_noise.grad = None
            val = mll(gp.MultivariateNormal(zeros, (A if B > 1 else A[0]) - floor), zeros)
            val.sum().backward()
            return val, lh.noise_covar.raw_noise.grad
        for N, k in DENSE:
            for B in (1, 3):
                cases = [(n, dense(N, k, c, B, dt)) for n, c in table(s)] + [("nan", with_nan(dense(N, k, None, B, dt), (B // 2, 2, 2)))]
                for n, A in cases:
                    case(f"factor/{tag}/N{N}/B{B}/{n}", "potrf", lambda: factor(A, given))
                    if given is None:
                        case(f"mll/{tag}/N{N}/B{B}/{n}", "mll_step", lambda: mll_value(A, B, N))
                case(f"psd_safe_cholesky/{tag}/N{N}/B{B}/rung1", "potrf", lambda: (gp.psd_safe_cholesky(cases[2][1], jitter=given),))
                case(f"psd_safe_cholesky/{tag}/N{N}/B{B}/upper", "potrf", lambda: (gp.psd_safe_cholesky(cases[0][1][0], upper=True),))
        # ---- ops.vk_forms
        V3, r3 = torch.tensor(V[keep]).to(dt), torch.tensor(r[keep]).to(dt)
        for n, c in table(s):
            Vc = V3.clone()
            if c is not None:
                Vc[1, 41] = Vc[1, 40] - c
            case(f"forms/{tag}/{n}", "vk_forms", lambda: gp._safe_forms(Vc.to(dev), r3.to(dev), given))
        case(f"forms/{tag}/nan", "vk_forms", lambda: gp._safe_forms(with_nan(V3, (0, 5)).to(dev), r3.to(dev), given))
        # ---- ops.markov_draw
        z, mean = z64.to(dt).to(dev), torch.zeros(1, H, dtype=F64, device=dev)

        def draw(diag):
            d = torch.tensor(diag[None]).to(dev)
            return gp._safe_draw(lambda j: ops.markov_draw(mean, d, d, z, j), (d, d, mean, z), given, f64=dt == F64)
        for n, c in table(s) + (("nan", None),):
            diag = 0.01 * (1.0 + np.arange(H))
            if c is not None:
                diag[32] = diag[31] - c
            if n == "nan":
                diag[7] = np.nan
            case(f"draw/{tag}/{n}", "markov_draw", lambda: draw(diag))
        if given is None:                                                     # through the model's lazy covariance, its own default
            for n, c in table(s):
                diag = 0.01 * (1.0 + np.arange(H))
                if c is not None:
                    diag[32] = diag[31] - c
                d = torch.tensor(diag).to(dev)
                case(f"markov_cov/{tag}/{n}", "markov_draw", lambda: (gp._MarkovCov(d, d, dtype=dt).draw(None, z),))
        # ---- the 1x1 covariance: its default first rung is the fp32 one whatever the dtype
        s1 = given if given is not None else 1e-6
        for n, c in table(s1) + (("nan", float("nan")),):
            pc = torch.tensor([1.0, 1.0 if c is None else -c, 2.0], dtype=dt, device=dev).reshape(3, 1, 1)
            case(f"chol_1x1/{tag}/{n}", None, lambda: (rollout_utils._chol_1x1(pc, given),))
    # ---- the quirk: a half-precision input is factored in fp32 and starts at the fp64 rung
    for n, c in (("clean", None), ("2^-24", 2.0 ** -24), ("2^-20", 2.0 ** -20), ("exhausted", 1.0)):
        case(f"factor/half/{n}", "potrf", lambda: factor(dense(8, 5, c, 1, torch.float16), None))
        case(f"factor/bfloat16/{n}", "potrf", lambda: factor(dense(8, 5, c, 1, torch.bfloat16), None))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--out", help="write the digests to this JSON file")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        A, B = (json.load(open(f)) for f in a.compare)
        bad = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
        print(f"{len(A)} and {len(B)} digests, {len(bad)} differ")
        for k in sorted(set(A) | set(B)):
            print("  ", "DIFFERS" if k in bad else "same   ", k, A.get(k, "-")[:16], B.get(k, "-")[:16])
        sys.exit(1 if bad or not A else 0)
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    d = digest_cases(torch, torch.device("cuda"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(d, fh, indent=0, sort_keys=True)
    print(json.dumps({"tree": os.path.abspath(a.tree), "digests": len(d), "cases_that_end_in_an_exception": RAISED,
                      "all": hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""A/B of the Markov-family and multi-task GPCV kernels (csrc/gpcv_markov.hip, gpcv_mt_markov.hip, markov_predict.hip,
gpcv_mt.hip, gpcv_mt_cv.hip and the headers they share) between two checkouts: same bits, same speed.

    python scripts/ab_markov_kernels.py --tree <checkout> --out digests.json     # SHA-256 of every output tensor
    python scripts/ab_markov_kernels.py --tree <checkout> --time                 # one JSON line of ms per call
    python scripts/ab_markov_kernels.py --compare a.json b.json                  # exit 1 unless every digest is equal

One process loads ONE library, so run it once per checkout (``--tree``: the checkout whose volt_amd is imported, default
this one; it must be built).  The cases are fixed and seeded on the host.  They are the smallest that reach every branch of
the shared device code: N around the lane, wave and chunk carries of the scans (chunk = 512 x 4 points; the root draw's is
256 x 4), B 1 / 3 / 65, T on both sides of the 256- / 1024-thread task workgroup and of the grouped / ungrouped G sums, Kc
0 / 1 / 5 / 8, Q below and above a wave, test points on the grid, between knots, before x_0, beyond x_{N-1} and duplicated,
S 1 / 64 / 65 with aligned and unaligned rows; and three failing inputs per family: a K_t whose first pivot is 0, a NaN in
rho, a NaN "cv" parameter.  The workspace arrays the ops expose (.s, the draw plan) are hashed too.  NaNs are canonicalised
before hashing; nothing else is: -0.0 is not 0.0.
--time runs the step / plan / draw legs of scripts/bench_gpcv_markov.py, bench_gpcv_mt_markov.py, bench_gpcv_predict.py and
bench_gpcv_multitask_cv.py at their committed shapes, with their inputs and their timing windows; run the two checkouts
alternately, each run a process of its own (profiles/markov_core/ab.txt).
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

SCAN_N = [1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097]
DRAW_N = [1023, 1024, 1025]
TS = [1, 3, 16, 17, 31, 32, 64]
KCS = [0, 1, 5, 8]
DENSE_N = [1, 5, 128, 129]
HS = [1, 31, 32, 33, 130]
SS = [1, 64, 65]


def digest(t):
    a = t.detach().cpu().contiguous().numpy()
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), np.array(np.nan, dtype=a.dtype), a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


class Cases:
    """Inputs drawn on the host from one seeded generator per case name, so that both checkouts see the same bytes."""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev

    def rng(self, name):
        return np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little"))

    def t(self, a):
        return self.torch.as_tensor(np.asarray(a), dtype=self.torch.float32).to(self.dev)

    def gh(self, Q):
        x, w = np.polynomial.hermite.hermgauss(Q)
        return self.t(x), self.t(w / np.sqrt(np.pi))

    def grid(self, r, N):
        return np.cumsum(r.uniform(0.5, 1.5, N)) / 252.0

    def abc(self, r, B, Kc):
        return np.stack([r.uniform(0.3, 1.3, (B, Kc)), r.uniform(0.1, 0.2, (B, Kc)), r.uniform(0.0, 1.0, (B, Kc))], 1)

    def single(self, name, B, N, Kc):
        r = self.rng(name)
        m = np.log(0.2) + 0.3 * r.standard_normal((B, N))
        return dict(x=self.grid(r, N), vol=r.uniform(0.05, 0.5, B), m=m, y=r.standard_normal((B, N)) * np.exp(m),
                    rho=3.0 + 0.1 * r.standard_normal((B, N)), gam=-0.5 + 0.1 * r.standard_normal((B, N)),
                    abc=self.abc(r, B, Kc) if Kc else None)

    def multi(self, name, N, T, Kc):
        r = self.rng(name)
        M = np.log(0.2) + 0.3 * r.standard_normal((N, T))
        return dict(x=self.grid(r, N), M=M, y=r.standard_normal((N, T)) * np.exp(M), rho=3.0 + 0.1 * r.standard_normal(N),
                    gam=-0.5 + 0.1 * r.standard_normal(N), Lt=np.tril(np.eye(T) + 0.1 * r.standard_normal((T, T))),
                    c=np.full(T, np.log(0.2)) + 0.05 * r.standard_normal(T), cf=0.1 * r.standard_normal(T),
                    rv=0.2 * r.standard_normal(T), abc=self.abc(r, T, Kc) if Kc else None,
                    Lx=np.tril(0.05 * np.eye(N) + 0.01 / np.sqrt(N) * r.standard_normal((N, N))))


def digest_cases(torch, ops, dev):
    c = Cases(torch, dev)
    out, failed = {}, {}

    def put(name, info, **tensors):
        torch.cuda.synchronize()
        for k, v in tensors.items():
            if v is not None:
                out[f"{name}/{k}"] = digest(v)
        out[f"{name}/info"] = digest(info)
        if bool((info != 0).any()):                                   # (reported, so that a run shows its failing cases ran)
            failed[name.split("/")[0]] = failed.get(name.split("/")[0], 0) + 1

    # ---- the single-task Markov step, root variance and root draw
    def markov_step(tag, B, N, Kc, Q, fail=None):
        p = c.single(f"single/{tag}", B, N, Kc)
        if fail == "rho":
            p["rho"][0, N // 2] = np.nan
        if fail == "abc":
            p["abc"][0, 1, 0] = np.nan
        T = {k: (c.t(v) if v is not None else None) for k, v in p.items()}
        ghx, ghw = c.gh(Q)
        ws = ops.gpcv_markov_step(T["x"], T["vol"], T["m"] - float(np.log(0.2)), T["m"], T["rho"], T["gam"], T["y"], ghx, ghw,
                                  abc=T["abc"], w_ell=1.0 / N, w_kl=1.0 / N)
        put(f"gpcv_markov_step/{tag}", ws.info, out=ws.out, grad_m=ws.grad_m, grad_mu=ws.grad_mu, grad_rho=ws.grad_rho,
            grad_gamma=ws.grad_gamma, grad_abc=ws.grad_abc if Kc else None, s=ws.s)
        if Kc == 0 and Q == 20:
            var = ops.markov_root_var(T["rho"], T["gam"])
            out[f"markov_root_var/{tag}"] = digest(var)
            if fail is None:
                out[f"markov_root_var_equals_step_s/{tag}"] = str(bool(torch.equal(var, ws.s)))
            for reps in (1, 2):
                eps = c.t(c.rng(f"eps/{tag}/{reps}").standard_normal((B, reps, N)))
                out[f"markov_root_draw/{tag}/reps{reps}"] = digest(ops.markov_root_draw(T["m"], T["rho"], T["gam"], eps))

    for N in SCAN_N + DRAW_N:
        for B, Kc, Q in ((1, 0, 20), (3, 5, 20), (3, 1, 75), (1, 8, 20), (3, 0, 75)):
            markov_step(f"{B}x{N}/K{Kc}/Q{Q}", B, N, Kc, Q)
    for N in (65, 513):
        for Kc in (0, 5):
            markov_step(f"65x{N}/K{Kc}/Q20", 65, N, Kc, 20)
    markov_step("3x513/K0/Q20/nan_rho", 3, 513, 0, 20, fail="rho")
    markov_step("3x513/K5/Q20/nan_abc", 3, 513, 5, 20, fail="abc")

    # ---- the multi-task Markov step
    def mt_markov(tag, N, T, Kc, Q, fail=None):
        p = c.multi(f"multi/{tag}", N, T, Kc)
        if fail == "pivot":
            p["cf"][:] = 0.0
            p["rv"][:] = -1e4                                          # softplus -> 0: K_t = 0, the first pivot is 0
        if fail == "rho":
            p["rho"][N // 2] = np.nan
        if fail == "abc":
            p["abc"][0, 1, 0] = np.nan
        D = {k: (c.t(v) if v is not None else None) for k, v in p.items()}
        ghx, ghw = c.gh(Q)
        ws = ops.gpcv_mt_markov_step(D["x"], c.t([0.2]), D["M"], D["c"], D["rho"], D["gam"], D["Lt"], D["cf"], D["rv"], D["y"], ghx,
                                     ghw, abc=D["abc"], w_ell=1.0 / N, w_kl=1.0 / (N * T))
        put(f"gpcv_mt_markov_step/{tag}", ws.info, out=ws.out, grad_M=ws.grad_M, grad_c=ws.grad_c, grad_rho=ws.grad_rho,
            grad_gamma=ws.grad_gamma, grad_Lt=ws.grad_Lt, grad_cf=ws.grad_covar_factor, grad_rv=ws.grad_raw_var,
            grad_abc=ws.grad_abc if Kc else None, s=ws.s)
        if Kc == 0 and fail is None:
            var = ops.markov_root_var(D["rho"][None], D["gam"][None])[0]
            out[f"markov_root_var_equals_mt_s/{tag}"] = str(bool(torch.equal(var, ws.s)))

    for N in SCAN_N:
        for T, Kc in ((3, 0), (17, 5)):
            mt_markov(f"{N}x{T}/K{Kc}/Q20", N, T, Kc, 20)
    for N in (65, 513, 4097):
        for T in TS:
            for Kc, Q in ((0, 75), (1, 20), (8, 20)):
                mt_markov(f"{N}x{T}/K{Kc}/Q{Q}", N, T, Kc, Q)
    mt_markov("513x17/K0/Q20/zero_pivot", 513, 17, 0, 20, fail="pivot")
    mt_markov("513x17/K0/Q20/nan_rho", 513, 17, 0, 20, fail="rho")
    mt_markov("513x17/K5/Q20/nan_abc", 513, 17, 5, 20, fail="abc")

    # ---- the dense multi-task steps ("exp": Kc = 0, and "cv")
    def mt_dense(tag, N, T, Kc, fail=None):
        p = c.multi(f"dense/{tag}", N, T, Kc)
        if fail == "pivot":
            p["cf"][:] = 0.0
            p["rv"][:] = -1e4
        if fail == "abc":
            p["abc"][0, 1, 0] = np.nan
        D = {k: (c.t(v) if v is not None else None) for k, v in p.items()}
        K = 0.2 * torch.minimum(D["x"][:, None], D["x"][None, :])
        ghx, ghw = c.gh(20)
        ws = ops.gpcv_mt_step(K, D["M"], D["c"], D["Lx"], D["Lt"], D["cf"], D["rv"], D["y"], ghx, ghw, want_dk=True, abc=D["abc"],
                              w_ell=1.0 / N, w_kl=1.0 / (N * T))
        put(f"gpcv_mt_step/{tag}", ws.info, out=ws.out, grad_M=ws.grad_M, grad_c=ws.grad_c, grad_Lx=ws.grad_Lx, grad_Lt=ws.grad_Lt,
            grad_cf=ws.grad_covar_factor, grad_rv=ws.grad_raw_var, grad_K=ws.grad_K, grad_abc=ws.grad_abc if Kc else None)

    for N in DENSE_N:
        for T in TS:
            for Kc in KCS:
                mt_dense(f"{N}x{T}/K{Kc}", N, T, Kc)
    mt_dense("129x17/K0/zero_pivot", 129, 17, 0, fail="pivot")
    mt_dense("129x17/K5/zero_pivot", 129, 17, 5, fail="pivot")
    mt_dense("129x17/K5/nan_abc", 129, 17, 5, fail="abc")

    # ---- prediction away from the grid: plan and draw
    def points(r, x, H):
        """on the grid, between knots, before x_0, beyond x_{N-1}, duplicated -- in the caller's (unsorted) order"""
        N = len(x)
        kinds = [x[r.integers(0, N, H)], r.uniform(0.0, x[0], H), r.uniform(x[-1], 1.3 * x[-1] + 0.01, H),
                 r.uniform(x[0], x[-1] + 1e-6, H)]
        xs = np.array([kinds[h % 4][h] for h in range(H)], dtype=np.float32)
        if H > 2:
            xs[H // 2] = xs[0]                                         # a duplicate
        return xs

    def predict(tag, B, N, H, fail=None):
        p = c.single(f"predict/{tag}", B, N, 0)
        r = c.rng(f"predict_xs/{tag}")
        xs = points(r, p["x"].astype(np.float32), H)
        if fail == "rho":
            p["rho"][0, N // 2] = np.nan
        T = {k: (c.t(v) if v is not None else None) for k, v in p.items()}
        plan = ops.markov_predict_plan(T["x"], c.t(xs), T["vol"], c.t(np.full(B, np.log(0.2))), T["m"], T["rho"], T["gam"])
        put(f"markov_predict_plan/{tag}", plan.info, mean=plan.mean, var_q=plan.var_q, var_p=plan.var_p, coef=plan.coef, code=plan.code,
            steps=plan.steps)
        if fail is None:
            var = ops.markov_root_var(T["rho"], T["gam"])
            out[f"markov_predict_plan/{tag}/s_last"] = digest(var[:, -1])
        for S in SS:
            for pad in (0, 1, 3):                                      # rows of eps of plan.E, + 1, + 3 columns: aligned or not
                eps = c.t(c.rng(f"predict_eps/{tag}/{S}/{pad}").standard_normal((B, S, plan.E + pad)))
                for ex, part in ((False, "both"), (True, "both"), (False, "chain"), (False, "bridge")):
                    out[f"markov_predict_draw/{tag}/S{S}/pad{pad}/exp{int(ex)}/{part}"] = digest(ops.markov_predict_draw(plan, eps, exp=ex, part=part))

    for N in SCAN_N:
        for B, H in ((1, 1), (3, 33), (3, 32)):
            predict(f"{B}x{N}/H{H}", B, N, H)
    for N in (65, 513):
        for H in HS:
            predict(f"3x{N}/H{H}b", 3, N, H)
        predict(f"65x{N}/H31", 65, N, 31)
    predict("3x513/H33/nan_rho", 3, 513, 33, fail="rho")
    return out, failed


def time_cases(torch, tree, rounds, only=None):
    """{leg: ms per call}: the step / plan / draw legs of the four benchmarks at their committed shapes"""
    sys.path.insert(0, os.path.join(tree, "scripts"))
    import bench_gpcv_linear as BL
    import bench_gpcv_markov as BM
    import bench_gpcv_mt_markov as BT
    import bench_gpcv_multitask_cv as BC
    import bench_gpcv_predict as BP
    from bench_bm_linear import prepare
    from bench_gpcv_multitask import _gh, _inputs, _mt_step_fn, _time
    from volt_amd import ops
    res = {}
    want = lambda name: not only or any(name.startswith(o) for o in only)

    def legs(prefix, arms, calls):
        arms = {k: v for k, v in arms.items() if want(f"{prefix}/{k}")}
        if arms:
            t = BL.alternate(arms, calls, rounds)
            for k in arms:
                res[f"{prefix}/{k}"] = t[k]

    for B, N in BM.SHAPES:
        for lik in ("exp", "cv"):
            if want(f"gpcv_markov_step/{B}x{N}/{lik}"):
                run, ws = BM.markov_step_arm(B, N, lik, 3)
                legs(f"gpcv_markov_step/{B}x{N}/{lik}", {"markov": run}, BL.window_calls(20, N))
                del run, ws
    for N, T in BT.SHAPES:
        for lik in ("exp", "cv"):
            if want(f"gpcv_mt_markov_step/{N}x{T}/{lik}"):
                arms, keep = BT.step_arms(N, T, lik, (N, T) not in BT.MARKOV_ONLY, 3)
                arms.pop("single")
                legs(f"gpcv_mt_markov_step/{N}x{T}/{lik}", arms, BL.window_calls(20, N))
                del arms, keep
                torch.cuda.empty_cache()
    for B, N in BP.SHAPES:
        if not want(f"markov_predict/{B}x{N}"):
            continue
        model, x = BP.model_of(B, N)
        for H, S in BP.POINTS:
            xs = BP.test_points(x, H)
            plan = model(xs).plan
            d = model.variational_strategy._variational_distribution
            flat = [t.detach().reshape(B, N) for t in (d.variational_mean, d.log_diag_precision_root, d.coupling)]
            vol, mu = model.covar_module.vol.detach().reshape(-1), model.mean_module.constant.detach().reshape(-1)
            eps = torch.randn(B, S, plan.E, device="cuda")
            arms = {"plan": prepare(lambda: ops.markov_predict_plan(x, xs, vol, mu, *flat), 3, True),
                    "draw": prepare(lambda: ops.markov_predict_draw(plan, eps), 3, True)}
            legs(f"markov_predict/{B}x{N}/H{H}/S{S}", arms, 5 if (N > 4096 or S > 1000) else 20)
            del arms, eps, plan
        del model
        torch.cuda.empty_cache()
    gx, gw = _gh()
    for n, T in ((399, 8), (399, 64), (4096, 8), (4096, 64)):
        if not want(f"gpcv_mt_step/{n}x{T}"):
            continue
        reps = 50 if n <= 1024 else (10 if T <= 8 else 4)
        _, _, K, Lq, m, y = _inputs(n, T)
        fns = {"exp": _mt_step_fn(n, T, K, Lq, m, y, gx, gw)[0], "cv_k1": BC._mt_cv_step_fn(n, T, 1, K, Lq, m, y, gx, gw),
               "cv_k5": BC._mt_cv_step_fn(n, T, 5, K, Lq, m, y, gx, gw)}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                t[k].append(_time(fn, reps))
        for k, v in t.items():
            res[f"gpcv_mt_step/{n}x{T}/{k}"] = round(float(np.median(v)), 5)
        del fns, K, Lq
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", help="write the digests (or, with --time, the timings) to this JSON file")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", nargs="*", metavar="LEG", help="with --time: only the legs whose names begin with one of these")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        A, B = (json.load(open(f)) for f in a.compare)
        bad = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
        print(f"{len(A)} and {len(B)} digests, {len(bad)} differ")
        for k in bad:
            print("  ", k, A.get(k), B.get(k))
        sys.exit(1 if bad or not A else 0)
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import torch
    from volt_amd import ops
    dev = torch.device("cuda")
    if a.time:
        line = {"tree": tree, "ms": time_cases(torch, tree, a.rounds, a.only)}
    else:
        d, failed = digest_cases(torch, ops, dev)
        line = {"tree": tree, "digests": len(d), "cases_with_nonzero_info": failed,
                "all": hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(line["ms"] if a.time else d, fh, indent=0, sort_keys=True)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

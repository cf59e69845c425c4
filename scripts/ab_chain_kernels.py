#!/usr/bin/env python
"""A/B of the chain kernels (csrc/bm.hip, gpcv_bm.hip, chain_draw.hip) between two checkouts: same bits, same speed.

    python scripts/ab_chain_kernels.py --tree <checkout> --out digests.json     # SHA-256 of every output tensor
    python scripts/ab_chain_kernels.py --tree <checkout> --time                 # one JSON line of ms per call
    python scripts/ab_chain_kernels.py --compare a.json b.json                  # exit 1 unless every digest is equal

One process loads ONE library, so run it once per checkout (``--tree``: the checkout whose volt_amd is imported, default
this one; it must be built).  The cases are fixed and seeded on the host: fp32 and fp64, gradient on and off, shared and
per-series grids, jitter 0 and > 0, the edge sizes of the GPU tests (N 1 .. 399, B 1 .. 130, H 1 .. 130) plus 8 x 4096 and
64 x 399, and one failing pivot per op.  NaNs are canonicalised before hashing; nothing else is: -0.0 is not 0.0.
--time follows profiles/host_plumbing/ab.txt: run the two checkouts alternately, each run a process of its own.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

EDGES = [(1, 1), (3, 2), (1, 3), (3, 31), (65, 32), (3, 33), (1, 63), (130, 64), (3, 65), (65, 129), (65, 399)]
LARGE = [(8, 4096), (64, 399)]
HS = [1, 20, 65, 130]


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

    def t(self, a, dt):
        return self.torch.as_tensor(np.asarray(a), dtype=dt).to(self.dev)

    def chain(self, name, B, N, dt, per_series=False, fail=False):
        """grid (increasing, x_0 > 0; [B,N] when per_series), vol, sigma2, resid.  fail: series 0 gets a negative noise, so its
        first pivot v x_0 + s is negative."""
        r = self.rng(name)
        x = np.cumsum(r.uniform(0.5, 1.5, size=(B, N) if per_series else N), axis=-1) / 252.0
        vol, s2 = r.uniform(0.05, 0.5, B), r.uniform(1e-3, 0.2, B)
        if fail:
            s2[0] = -1.0
        return self.t(x, dt), self.t(vol, dt), self.t(s2, dt), self.t(r.standard_normal((B, N)), dt)


def digest_cases(torch, ops, dev):
    c = Cases(torch, dev)
    f32, f64 = torch.float32, torch.float64
    out, failed = {}, {}

    def put(name, **tensors):
        torch.cuda.synchronize()
        for k, v in tensors.items():
            out[f"{name}/{k}"] = digest(v)
        if bool((tensors["info"] != 0).any()):                                    # (reported, so that a run shows its failing-pivot cases ran)
            failed[name.split("/")[0]] = failed.get(name.split("/")[0], 0) + 1

    for dt, dn in ((f32, "f32"), (f64, "f64")):
        for B, N in EDGES + LARGE:
            for fail in ((False, True) if (B, N) == (3, 65) else (False,)):
                tag = f"{dn}/{B}x{N}" + ("/fail" if fail else "")
                x, vol, s2, r = c.chain(f"chain/{tag}", B, N, dt, fail=fail)
                V, _, _, _ = c.chain(f"chain_v/{tag}", B, N, dt, per_series=True)
                for grad in (True, False):
                    cols = slice(None) if grad else [0, 2, 3, 6, 7]          # the gradient columns are not written without it
                    o, al, info = ops.bm_step(x, vol, s2, r, want_grad=grad)
                    put(f"bm_step/{tag}/grad{int(grad)}", out=o[:, cols], info=info, **({"alpha": al} if grad else {}))
                    for gname, grid in (("shared", x), ("own", V)):
                        o, al, info = ops.vk_step(grid, s2, r, want_grad=grad)
                        put(f"vk_step/{tag}/{gname}/grad{int(grad)}", out=o[:, cols], info=info, **({"alpha": al} if grad else {}))
                for gname, grid in (("shared", x), ("own", V)):
                    for jit in (0.0, 1e-3):
                        j = torch.full((B,), jit, dtype=f64, device=dev)
                        if fail:
                            j[0] = -1.0
                        o, info = ops.vk_forms(grid, j, r)
                        put(f"vk_forms/{tag}/{gname}/jit{jit}", out=o, info=info)
                for H in (HS if N <= 129 else [20]):
                    xs = torch.sort(c.t(c.rng(f"xs/{tag}/{H}").uniform(0.0, 1.3 * float(x[-1]), H), dt)).values
                    for gname, grid in (("shared", x), ("own", V)):
                        o, info = ops.bm_post(grid, xs, vol, s2, r)
                        put(f"bm_post/{tag}/{gname}/H{H}", out=o, info=info)
                    R = c.t(c.rng(f"R/{tag}/{H}").standard_normal((B, N, H)), dt)
                    X, info = ops.bm_solve(x, vol, s2, R)
                    put(f"bm_solve/{tag}/H{H}", X=X, info=info)

    gh_x, gh_w = np.polynomial.hermite.hermgauss(20)
    ghx, ghw = c.t(gh_x, f32), c.t(gh_w / np.sqrt(np.pi), f32)
    for B, N in [(1, 1), (3, 2), (3, 33), (3, 65), (2, 129), (3, 399), (64, 399), (8, 4096)]:
        for jit in ((1e-3, 1e-2, -1.0) if (B, N) == (3, 65) else (1e-3,)):            # (the entry's jitter is > 0; -1: the failing pivot)
            tag = f"{B}x{N}/jit{jit}"
            r = c.rng(f"gpcv/{tag}")
            x, vol, _, resid = c.chain(f"gpcv_chain/{tag}", B, N, f32)
            m, y = c.t(r.standard_normal((B, N)) * 0.3, f32), c.t(r.standard_normal((B, N)) * 0.01, f32)
            Lq = torch.tril(c.t(r.standard_normal((B, N, N)) * (0.1 / np.sqrt(N)), f32)) + 0.5 * torch.eye(N, device=dev)
            ws = ops.gpcv_bm_step(x, vol, resid, m, Lq, y, ghx, ghw, jitter=jit, w_ell=1.0 / N, w_kl=1.0 / N)
            if jit < 0:
                put(f"gpcv_bm_step/{tag}", out=ws.out, info=ws.info)
            else:
                put(f"gpcv_bm_step/{tag}", out=ws.out, info=ws.info, grad_m=ws.grad_m, grad_mu=ws.grad_mu, grad_Lq=ws.grad_Lq)
            del ws, Lq

    for dt, dn in ((f32, "f32"), (f64, "f64")):
        for G, S, H in [(1, 1, 1), (3, 65, 20), (2, 130, 65), (3, 1000, 33), (2, 64, 130), (64, 1000, 20)]:
            for jit in (0.0, 1e-6):
                for fail in ((False, True) if (G, S, H) == (3, 65, 20) else (False,)):
                    tag = f"{dn}/{G}x{S}x{H}/jit{jit}" + ("/fail" if fail else "")
                    r = c.rng(f"draw/{tag}")
                    diag = np.cumsum(r.uniform(0.5, 1.5, (G, H)), axis=1) * 0.01
                    off = diag * r.uniform(0.8, 1.0, (G, H))
                    if fail:
                        diag[0, H // 2] = -1.0 if jit else 0.0                    # (jitter 0: a zero pivot; else a negative one)
                        diag[0, H // 2 + 1:] = 0.0
                    mean = c.t(r.standard_normal((G, H)), f64)
                    z = c.t(r.standard_normal((G, S, H)), dt)
                    for ex in (False, True):
                        o, info = ops.markov_draw(mean, c.t(diag, f64), c.t(off, f64), z, jitter=jit, exp=ex)
                        put(f"markov_draw/{tag}/exp{int(ex)}", out=o, info=info)
                    pv = c.t(r.uniform(0.05, 0.5, (G, S, H)), dt)
                    vlr = -1.0 if fail else 0.02                                    # W_0 + jitter < 0: the first pivot fails
                    for reps in (1, 2):
                        z2 = c.t(r.standard_normal((G, S * reps, H)), dt)
                        o, info = ops.vk_draw(pv, 0.2, vlr, 1.0 / 252, mean, z2, jitter=jit, reps=reps)
                        put(f"vk_draw/{tag}/reps{reps}", out=o, info=info)
    return out, failed


def time_cases(torch, ops, dev, repeats, target_ms, only=None):
    c = Cases(torch, dev)
    f32, f64 = torch.float32, torch.float64
    res = {}

    def leg(name, fn):
        if only and not any(name.startswith(o) for o in only):
            return
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(), fn(), b.record()
        torch.cuda.synchronize()
        iters = int(max(5, min(400, target_ms / max(a.elapsed_time(b), 1e-3))))
        ms = []
        for _ in range(repeats):
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / iters)
        res[name] = round(float(np.median(ms)), 5)

    for dt, dn in ((f32, "f32"), (f64, "f64")):
        for B, N in [(64, 399), (8, 4096), (1, 65536)]:
            tag = f"{dn}/{B}x{N}"
            x, vol, s2, r = c.chain(f"t/{tag}", B, N, dt)
            V, _, _, _ = c.chain(f"tv/{tag}", B, N, dt, per_series=True)
            j = torch.full((B,), 1e-3, dtype=f64, device=dev)
            ws = ops.BmWorkspace(B, N, dev, dt)
            for grad in (True, False):
                leg(f"bm_step/{tag}/grad{int(grad)}", lambda: ops.bm_step(x, vol, s2, r, ws, want_grad=grad))
                leg(f"vk_step/{tag}/grad{int(grad)}", lambda: ops.vk_step(V, s2, r, ws, want_grad=grad))
            leg(f"vk_forms/{tag}", lambda: ops.vk_forms(V, j, r))
            xs = torch.sort(c.t(c.rng("txs").uniform(0.0, 1.3 * float(x[-1]), 20), dt)).values
            leg(f"bm_post/{tag}/H20", lambda: ops.bm_post(x, xs, vol, s2, r))
            R = c.t(c.rng(f"tR/{tag}").standard_normal((B, N, 20)), dt)
            ws2 = ops.BmWorkspace(B, N, dev, dt, 20)
            leg(f"bm_solve/{tag}/H20", lambda: ops.bm_solve(x, vol, s2, R, ws2))
    gh_x, gh_w = np.polynomial.hermite.hermgauss(20)
    ghx, ghw = c.t(gh_x, f32), c.t(gh_w / np.sqrt(np.pi), f32)
    for B, N in [(64, 399), (8, 4096)]:
        r = c.rng(f"tg/{B}x{N}")
        x, vol, _, resid = c.chain(f"tgc/{B}x{N}", B, N, f32)
        m, y = c.t(r.standard_normal((B, N)) * 0.3, f32), c.t(r.standard_normal((B, N)) * 0.01, f32)
        Lq = torch.tril(c.t(r.standard_normal((B, N, N)) * (0.1 / np.sqrt(N)), f32)) + 0.5 * torch.eye(N, device=dev)
        ws = ops.GpcvBmWorkspace(B, N, dev, 0)
        leg(f"gpcv_bm_step/{B}x{N}", lambda: ops.gpcv_bm_step(x, vol, resid, m, Lq, y, ghx, ghw, ws, w_ell=1.0 / N, w_kl=1.0 / N))
        del ws, Lq
    G, S, H = 64, 1000, 20
    for dt, dn in ((f32, "f32"), (f64, "f64")):
        r = c.rng(f"td/{dn}")
        diag = np.cumsum(r.uniform(0.5, 1.5, (G, H)), axis=1) * 0.01
        dg, of, mean = c.t(diag, f64), c.t(diag * r.uniform(0.8, 1.0, (G, H)), f64), c.t(r.standard_normal((G, H)), f64)
        z, pv = c.t(r.standard_normal((G, S, H)), dt), c.t(r.uniform(0.05, 0.5, (G, S, H)), dt)
        o, info = torch.empty_like(z), torch.empty(G, dtype=torch.int32, device=dev)
        info2 = torch.empty(G, S, dtype=torch.int32, device=dev)
        leg(f"markov_draw/{dn}/{G}x{S}x{H}", lambda: ops.markov_draw(mean, dg, of, z, 1e-6, out=o, info=info))
        leg(f"vk_draw/{dn}/{G}x{S}x{H}", lambda: ops.vk_draw(pv, 0.2, 0.02, 1.0 / 252, mean, z, 1e-6, out=o, info=info2))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", help="write the digests to this JSON file")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-ms", type=float, default=60.0, help="device time per timed repeat")
    ap.add_argument("--only", nargs="*", metavar="OP", help="with --time: only the legs whose names begin with one of these")
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
    from volt_amd import ops
    dev = torch.device("cuda")
    if a.time:
        print(json.dumps({"tree": os.path.abspath(a.tree), "ms": time_cases(torch, ops, dev, a.repeats, a.target_ms, a.only)}))
    else:
        d, failed = digest_cases(torch, ops, dev)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(d, fh, indent=0, sort_keys=True)
        print(json.dumps({"tree": os.path.abspath(a.tree), "digests": len(d), "cases_with_a_failed_pivot": failed,
                          "all": hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()

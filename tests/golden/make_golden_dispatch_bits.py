"""Record, on the GPU, the bits every dispatch path of the library hands its caller, into dispatch_bits.json.

    python tests/golden/make_golden_dispatch_bits.py --record run1.json     # one process
    python tests/golden/make_golden_dispatch_bits.py --record run2.json     # a second, separate process
    python tests/golden/make_golden_dispatch_bits.py --merge run1.json run2.json     # rewrites dispatch_bits.json

The host side of libvolt_hip.so decides which schedule a shape runs and carves the caller's scratch; a change there that is
meant to leave every launch alone must leave every result bit alone.  For each case -- the smallest shape that takes one path
-- the table holds the sha256 of what the call returned (out, alpha, info and the factor left in the workspace; A, Winv, Y for
the factorisation entries).  A case enters the table only if two separate processes gave the same digests; one that did
not (only the K-sliced paths may: their slabs are summed in arrival order) is listed under `omitted` with both.
tests/test_gpu_dispatch_bits.py runs the same cases (`run_case`) and compares.

Which path a shape takes is confirmed here, not assumed (`--record` fails otherwise): the state region a one-launch step
needs is in the workspace only where its gate lets the shape in, so the byte queries with that step switched off
(VOLT_TUNE=1 children, host only) tell which regions a workspace holds, and mll.hip tries them in the order long series,
short series, batched; volt_profile_step_f32's launch counts ([1, 0]) confirm the batched one-launch step on the device.

The inputs are made of integers (numpy's bit generator, exact scalings by powers of two), so every machine builds the same
matrices bit for bit; their digests are in the table too, and the test checks them first."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dispatch_bits.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name: (kind, B, N, options, the path the shape must take)
CASES = {
    "f32_step_short_series": ("mll", 2, 300, {}, "small"),
    "f32_step_long_series": ("mll", 1, 500, {}, "long"),
    "f32_step_batched_local": ("mll", 8, 1280, {}, "batch"),
    "f32_step_batched_agent": ("mll", 6, 1280, {}, "batch"),
    "f32_step_plain_one_group": ("mll", 72, 384, {}, "columns"),
    "f32_step_plain_two_groups": ("mll", 144, 512, {}, "columns"),
    "f32_step_no_tables": ("mll", 2, 300, {"tables": False}, "columns"),
    "f32_step_forward_only": ("mll", 8, 1280, {"want_grad": False}, "batch"),
    "f32_step_refine_alpha": ("mll", 2, 300, {"refine_alpha": True}, "small"),
    "f32_potrf_scratch": ("potrf", 8, 1280, {}, "batch"),
    "f32_potrf_no_tables": ("potrf", 8, 1280, {"tables": False}, "columns"),
    "f32_potrf_two_call": ("potrf_two_call", 8, 1280, {}, "batch"),
    "f32_trtri": ("trtri", 2, 384, {}, None),
    "f64_step_one_launch": ("mll64", 1, 256, {}, "batch64"),
    "f64_step_one_launch_local": ("mll64", 8, 256, {}, "batch64"),
    "f64_potrf_one_launch": ("potrf64", 1, 256, {}, "batch64"),
    "f64_potrf_one_launch_local": ("potrf64", 8, 256, {}, "batch64"),
    "f64_trtri_workspace": ("trtri64", 2, 384, {}, "batch64"),
}
GROUPS = {"f32_step_plain_one_group": 1, "f32_step_plain_two_groups": 2}     # stream groups of the launch-per-column cases
LOCAL = {"f32_step_batched_local": True, "f32_step_batched_agent": False, "f32_step_forward_only": True, "f32_potrf_scratch": True,
         "f64_step_one_launch": False, "f64_step_one_launch_local": True, "f64_potrf_one_launch": False,
         "f64_potrf_one_launch_local": True}                                  # hand-offs through the XCD's L2


def inputs(B, N, dtype=np.float32):
    """K [B,N,N] symmetric positive definite, resid [B,N], sigma2 [B]: integers scaled by powers of two (exact in fp32).
    Off-diagonal entries uniform in +-1/32 (spectral radius ~ 0.036 sqrt(N) < 1.3 at N = 1280) under a diagonal in [3, 4):
    no structure below the diagonal, condition number below 10."""
    rng = np.random.default_rng([B, N])
    low = np.tril(rng.integers(-128, 128, size=(B, N, N), dtype=np.int32), -1)
    K = (low + np.swapaxes(low, -1, -2)).astype(dtype) / dtype(4096)
    idx = np.arange(N)
    K[:, idx, idx] = dtype(3) + rng.integers(0, 256, size=(B, N)).astype(dtype) / dtype(256)
    r = rng.integers(-256, 256, size=(B, N)).astype(dtype) / dtype(64)
    s2 = (1 + np.arange(B) % 8).astype(dtype) / dtype(16)
    return K, r, s2


def sha(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().contiguous().numpy()
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def _workspace_matrix(ws, B, N, torch, dtype):
    """The factor the step left at the head of its workspace (csrc/mll.hip, mll64.hip: A comes first), lower triangle."""
    from volt_amd import ops
    Np = ops.padded_n(N)
    off = ws.ptr - ws.buf.data_ptr()
    A = ws.buf[off: off + B * Np * Np * torch.empty(0, dtype=dtype).element_size()].view(dtype).view(B, Np, Np)
    return torch.tril(A[:, :N, :N])


def run_case(name):
    """Run one case on the current device; {what: sha256}, the inputs' digest included."""
    import torch
    from volt_amd import _lib, ops
    kind, B, N, opt, _path = CASES[name]
    L = _lib.lib()
    f64 = kind.endswith("64")
    tdt = torch.float64 if f64 else torch.float32
    Kh, rh, sh = inputs(B, N, np.float64 if f64 else np.float32)
    d = {"inputs": sha(Kh) + sha(rh)[:16] + sha(sh)[:16]}
    K, r, s2 = torch.from_numpy(Kh).cuda(), torch.from_numpy(rh).cuda(), torch.from_numpy(sh).cuda()
    st = _lib.stream_ptr()
    if kind in ("mll", "mll64"):
        wg = opt.get("want_grad", True)
        ws = ops.MllWorkspace(B, N, wg, K.device, tdt)
        ws.buf.zero_()                                   # what a step does not write is the same in every process
        ws.out.zero_()
        ws.alpha.zero_()
        if not f64:
            _lib.check(L.volt_mll_workspace_init_f32(ws.ptr, B, N, int(wg), st), "init")
        ops.mll_step(K, r, s2, ws, want_grad=wg, refine_alpha=opt.get("refine_alpha", False), tables=opt.get("tables", True))
        d.update(out=sha(ws.out), alpha=sha(ws.alpha), info=sha(ws.info), factor=sha(_workspace_matrix(ws, B, N, torch, tdt)))
        assert int(ws.info.abs().sum()) == 0, name
    elif kind in ("potrf", "potrf64"):
        f = ops.potrf(K, s2, tables=opt.get("tables", True))
        d.update(A=sha(torch.tril(f.A[:, :N, :N])), Winv=sha(f.Winv), info=sha(f.info))
        assert int(f.info.abs().sum()) == 0, name
    elif kind == "potrf_two_call":
        Np = ops.padded_n(N)
        f = ops.potrf(K, s2)
        wp, nbytes = ops._potrf_workspace(B, Np, K.device)
        assert wp is not None
        A, W, info = torch.zeros_like(f.A), torch.zeros_like(f.Winv), torch.empty_like(f.info)
        _lib.check(L.volt_prepare_f32(K.data_ptr(), N, N * N, s2.data_ptr(), 0.0, A.data_ptr(), B, N, st), "prepare")
        _lib.check(L.volt_potrf_ws_f32(A.data_ptr(), W.data_ptr(), info.data_ptr(), B, Np, wp, nbytes, _lib.WS_INITIALISED, st), "potrf")
        assert torch.equal(torch.tril(A), torch.tril(f.A)) and torch.equal(W, f.Winv), name      # ... against volt_potrf_k_f32
        d.update(A=sha(torch.tril(A[:, :N, :N])), Winv=sha(W), info=sha(info))
    elif kind in ("trtri", "trtri64"):
        f = ops.potrf(K, s2)
        d.update(A=sha(torch.tril(f.A[:, :N, :N])), Winv=sha(f.Winv), Y=sha(ops.trtri(f)))
    else:
        raise ValueError(kind)
    return d


# ------------------------------------------------------------------ which path a shape takes
_KNOBS = {"default": {}, "no_batch": {"VOLT_BATCH": "0"}, "no_long": {"VOLT_LONG": "0"}, "no_small": {"VOLT_SMALL_NMAX": "0"},
          "no_batch64": {"VOLT_BATCH64": "0"}}


def _bytes_of_cases():
    from volt_amd import _lib, ops
    L = _lib.lib()
    topo = (ctypes.c_int * 7)()
    L.volt_topology_describe(topo)
    t = {"topology": list(topo)}
    for name, (kind, B, N, opt, _path) in CASES.items():
        Np, g = ops.padded_n(N), int(opt.get("want_grad", True))
        t[name] = {"mll": lambda: L.volt_mll_workspace_bytes(B, N, g), "mll64": lambda: L.volt_mll_workspace_bytes_f64(B, N, g),
                   "potrf": lambda: L.volt_potrf_workspace_bytes(B, Np), "potrf_two_call": lambda: L.volt_potrf_workspace_bytes(B, Np),
                   "potrf64": lambda: L.volt_potrf_workspace_bytes_f64(B, Np), "trtri": lambda: 0,
                   "trtri64": lambda: L.volt_trtri_workspace_bytes_f64(B, Np)}[kind]()
    return t


def confirm_paths(on_device):
    """Raise unless every case takes the path it is named for."""
    by = {}
    for knob, extra in _KNOBS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("VOLT_")}
        env.update({"VOLT_TUNE": "1"}, **extra)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--bytes"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise RuntimeError(out.stderr[-800:])
        by[knob] = json.loads(out.stdout.strip().splitlines()[-1])
    topo = by["default"]["topology"]
    assert topo[:2] == [256, 8] and topo[6] == 7, topo
    paths = {}
    for name, (kind, B, N, opt, want) in CASES.items():
        holds = {step: by["default"][name] != by["no_" + step][name] for step in ("long", "small", "batch", "batch64")}
        if not opt.get("tables", True):
            got = "columns"                              # nothing handed over that a one-launch step could run on
        elif kind == "mll":
            grad = opt.get("want_grad", True)
            got = "long" if holds["long"] and grad else "small" if holds["small"] and grad else "batch" if holds["batch"] else "columns"
        elif kind == "trtri":
            got = None
        else:
            got = "batch64" if holds["batch64"] else "batch" if holds["batch"] else "columns"
        assert got == want, (name, got, want, holds)
        n = -(-N // 128)
        if name in GROUPS:
            assert (1 if B * (n + 1) < topo[5] else 2) == GROUPS[name], name
        if name in LOCAL:
            assert (B % 8 == 0 and topo[1] == 8) == LOCAL[name], name
        paths[name] = got
    if on_device:
        import torch
        from volt_amd import _lib, ops
        for name in ("f32_step_batched_local", "f32_step_batched_agent", "f32_step_short_series", "f32_step_plain_one_group"):
            _kind, B, N, _opt, want = CASES[name]
            Kh, rh, sh = inputs(B, N)
            K, r, s2 = torch.from_numpy(Kh).cuda(), torch.from_numpy(rh).cuda(), torch.from_numpy(sh).cuda()
            ws = ops.MllWorkspace(B, N, True, K.device)
            ms_sum, ms_un, cnt = (ctypes.c_float * 2)(), (ctypes.c_float * 2)(), (ctypes.c_int * 2)()
            _lib.check(_lib.lib().volt_profile_step_f32(K.data_ptr(), N, N * N, r.data_ptr(), s2.data_ptr(), ws.out.data_ptr(), ws.alpha.data_ptr(),
                                                        ws.ptr, ws.info.data_ptr(), B, N, 0, _lib.stream_ptr(), ms_sum, ms_un, cnt, None), "profile")
            assert (list(cnt) == [1, 0]) == (want == "batch"), (name, list(cnt))
            paths[name] += f" (profile hook: {'the batched one launch' if want == 'batch' else 'not the batched step'}, launches {list(cnt)})"
    return paths


if __name__ == "__main__":
    if "--bytes" in sys.argv:
        print(json.dumps(_bytes_of_cases()))
    elif "--record" in sys.argv:
        dest = sys.argv[sys.argv.index("--record") + 1]
        rec = {"paths": confirm_paths(on_device=True), "digests": {}}
        for name in CASES:
            rec["digests"][name] = run_case(name)
            print(name, rec["digests"][name], flush=True)
        with open(dest, "w") as fh:
            json.dump(rec, fh, indent=1)
    elif "--merge" in sys.argv:
        i = sys.argv.index("--merge")
        with open(sys.argv[i + 1]) as fa, open(sys.argv[i + 2]) as fb:
            a, b = json.load(fa), json.load(fb)
        table = {"paths": a["paths"], "cases": {}, "omitted": {}}
        for name in CASES:
            if a["digests"][name] == b["digests"][name]:
                table["cases"][name] = a["digests"][name]
            else:
                table["omitted"][name] = {"first_process": a["digests"][name], "second_process": b["digests"][name]}
        with open(OUT, "w") as fh:
            json.dump(table, fh, indent=1)
            fh.write("\n")
        print(OUT, "cases", len(table["cases"]), "omitted", sorted(table["omitted"]))
    else:
        raise SystemExit(__doc__)

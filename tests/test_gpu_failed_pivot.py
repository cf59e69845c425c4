"""info[b] -- 0, or the 1-based index of the first non-positive / NaN pivot (include/volt_hip.h) -- on every fp32 dispatch path.

Every safe_* route, psd_safe_cholesky, the MLL's jitter ladder and deferred_checks act on that one number.  A wrong index is
harmless; a missed failure sends a factor full of NaN into rollouts and gradients, a spurious one sends a healthy series up
the jitter ladder.  The matrices are tests/pivot_cases.py's: the integer-valued SPD inputs of the dispatch-bits table with one
row edited so that pivot i fails -- a negative diagonal, a pivot that fails only through the Schur complement (positive
diagonal, sum L_ij^2 beyond it: the only way a real covariance fails), an exactly zero pivot, a NaN on the diagonal, a NaN
below it -- at the borders of the 32-pivot phases and of the 128-tiles, in a middle tile, in the last tile and at the last
valid row of a ragged N.  The reference is the fp64 restatement of the header's definition (pivot_cases.first_failed_pivot):
tests/test_pivot_cases_host.py shows on the CPU that it gives i + 1 for every matrix planted here, with margins that make
i + 1 the answer in fp32 arithmetic too.

Per path (pivot_cases.PATHS; the schedule a shape runs is confirmed first, `schedules`):
  (a) every (i, kind): info == i + 1 for the planted series, 0 for the others; batches of 6 and more carry different cases in up
      to half their series at once, the even and the odd series taking turns;
  (b) the clean series of such a call return the bits of a call without failures on the same workspace;
  (c) after the failing calls the clean batch gives the clean bits again, info all 0;
  (d) two failures in one matrix: the smaller index is reported;
  (e) the outputs of a failed series: every path leaves NaN in out[b,0] and, with the gradient, in all of alpha[b,:]; the
      factorisation entries leave NaN at the failed pivot's own L[i,i] (include/volt_hip.h says so next to the info convention);
  (f) no call with a failed series runs into a hand-off time-out.  A waiter gives up after 3 s of wall clock
      (csrc/handoff.h VOLT_WAIT_TICKS) and reports it only where info is still 0, so on a failed series a time-out is
      invisible in info -- but not on the clock: every call here is a few milliseconds of work, and one that returns within
      half the time-out cannot have sat one out.  (The batched gradient step did: its diagonal tiles of the inverse waited for
      W_i's first word -- a float's bits, NaN of either sign for a failed series -- to be >= 1 as an integer.)
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import pivot_cases as pc
from test_gpu_contract import ops  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.0                                            # what the outputs hold before a call: tells "not written" from a value
HALF_A_TIMEOUT = 1.5                                         # seconds: half of csrc/handoff.h's VOLT_WAIT_TICKS

_CHILD = ("import json, sys\nfrom volt_amd import _lib, ops\nL = _lib.lib()\n"
          "print(json.dumps([[int(L.volt_mll_workspace_bytes(B, N, g)), int(L.volt_potrf_workspace_bytes(B, ops.padded_n(N)))]"
          " for B, N, g in json.loads(sys.argv[1])]))\n")
_KNOBS = {"default": {}, "no_batch": {"VOLT_BATCH": "0"}, "no_long": {"VOLT_LONG": "0"}, "no_small": {"VOLT_SMALL_NMAX": "0"}}


@pytest.fixture(scope="module")
def schedules(ops):
    """{path: the schedule its shape runs}, confirmed and printed once.  As make_golden_dispatch_bits.confirm_paths: the state
    of a one-launch step is in a workspace only where its gate lets the shape in, so the byte queries of processes with that step
    switched off (VOLT_TUNE=1 children, host only, started side by side) tell which regions a workspace holds; mll.hip tries
    them in the order long series, short series, batched.  Scratch without one-launch state runs the launch-per-column
    schedules: K-sliced throughout below 3 matrices (chol.hip run_factor_groups).  The gradient steps are then asked on the
    device: volt_profile_step_f32 counts ONE launch exactly for the batched step."""
    from volt_amd import _lib
    L = _lib.lib()
    names = list(pc.PATHS)
    arg = json.dumps([[B, N, int(opt.get("want_grad", True))] for _e, B, N, opt, _s, _f in pc.PATHS.values()])
    procs = {}
    for knob, extra in _KNOBS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("VOLT_")}
        env.update({"VOLT_TUNE": "1"}, **extra)
        procs[knob] = subprocess.Popen([sys.executable, "-c", _CHILD, arg], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)
    by = {}
    for knob, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, se[-800:]
        by[knob] = dict(zip(names, json.loads(so.strip().splitlines()[-1])))
    got = {}
    for name, (entry, B, N, opt, want, _full) in pc.PATHS.items():
        col = 0 if entry == "mll" else 1
        holds = {step: by["default"][name][col] != by["no_" + step][name][col] for step in ("long", "small", "batch")}
        grad = opt.get("want_grad", True)
        if not opt.get("tables", True) or entry == "plain":
            sched = "columns"                                # nothing handed over that a one-launch step could run on
        elif entry == "mll":
            sched = "long" if holds["long"] and grad else "small" if holds["small"] and grad else "batch" if holds["batch"] else "columns"
        else:
            sched = "batch" if holds["batch"] else "split" if by["default"][name][1] > 0 and B < 3 else "columns"
        how = "byte queries"
        if entry == "mll" and grad and opt.get("tables", True):
            Kh, rh, sh = pc.clean(B, N)
            K, r, s2 = (torch.tensor(x).cuda() for x in (Kh, rh, sh))
            ws = ops.MllWorkspace(B, N, True, K.device)
            ms_sum, ms_un, cnt = (ctypes.c_float * 2)(), (ctypes.c_float * 2)(), (ctypes.c_int * 2)()
            _lib.check(L.volt_profile_step_f32(K.data_ptr(), N, N * N, r.data_ptr(), s2.data_ptr(), ws.out.data_ptr(), ws.alpha.data_ptr(),
                                               ws.ptr, ws.info.data_ptr(), B, N, 0, _lib.stream_ptr(), ms_sum, ms_un, cnt, None), "profile")
            assert (list(cnt) == [1, 0]) == (sched == "batch"), (name, list(cnt))
            how += f"; profile hook: launches {list(cnt)}"
        if sched == "batch":
            local = B % 8 == 0
            assert local == ("agent" not in name), name
            sched += " (XCD-local hand-offs)" if local else " (agent-scope hand-offs)"
        assert sched.split()[0] == want, (name, sched, want, holds)
        got[name] = sched
        print(f"path {name}: {entry} ({B}, {N}) {opt or ''} -> {sched}  [{how}]")
    return got


class _Runner:
    """One path: its inputs on the device, its workspace, and `run(K)` -> (compared outputs ..., info)."""

    def __init__(self, ops, name):
        from volt_amd import _lib
        self.ops, self.lib, self.L, self.name = ops, _lib, _lib.lib(), name
        self.entry, self.B, self.N, self.opt, _sched, self.full = (pc.PATHS.get(name) or pc.TUNED_PATHS[name])[:6]
        Kh, rh, sh = pc.clean(self.B, self.N)
        self.Kh, self.sh = Kh, sh
        self.K, self.r, self.s2 = (torch.tensor(x).cuda() for x in (Kh, rh, sh))
        self.slowest = 0.0                                   # seconds of the longest call so far
        self.Np = ops.padded_n(self.N)
        if self.entry == "mll":
            self.wg = self.opt.get("want_grad", True)
            self.ws = ops.MllWorkspace(self.B, self.N, self.wg, self.K.device)

    def planted(self, plants):
        """The clean batch on the device with rows edited: plants = [(series, matrix from pivot_cases.plant, rows edited)]."""
        K = self.K.clone()
        for b, Kp, rows in plants:
            for i in rows:
                K[b, i, : i + 1] = torch.from_numpy(Kp[i, : i + 1]).cuda()
        return K

    def run(self, K):
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = self._run(K)
            torch.cuda.synchronize()
            self.slowest = max(self.slowest, time.perf_counter() - t0)
            return res
        except RuntimeError as e:                            # a HIP error: nothing more is started on a GPU that has faulted
            if "HIP" in str(e) or "hip" in str(e):
                pytest.exit(f"GPU error on path {self.name}: {e}", returncode=3)
            raise

    def _run(self, K):
        ops, L, st = self.ops, self.L, self.lib.stream_ptr()
        B, N, Np = self.B, self.N, self.Np
        if self.entry == "mll":
            self.ws.out.fill_(SENTINEL)
            self.ws.alpha.fill_(SENTINEL)
            ops.mll_step(K, self.r, self.s2, self.ws, want_grad=self.wg, refine_alpha=self.opt.get("refine_alpha", False),
                         tables=self.opt.get("tables", True))
            return self.ws.out.clone(), self.ws.alpha.clone(), self.ws.info.clone()
        if self.entry == "potrf":
            f = ops.potrf(K, self.s2, tables=self.opt.get("tables", True))
            return torch.tril(f.A), f.Winv, f.info
        A = torch.full((B, Np, Np), SENTINEL, device="cuda")
        W = torch.full((B, Np // 128, 128, 128), SENTINEL, device="cuda")
        info = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        self.lib.check(L.volt_prepare_f32(K.data_ptr(), N, N * N, self.s2.data_ptr(), 0.0, A.data_ptr(), B, N, st), "prepare")
        if self.entry == "two_call":
            wp, nbytes = ops._potrf_workspace(B, Np, K.device)
            assert wp is not None
            self.lib.check(L.volt_potrf_ws_f32(A.data_ptr(), W.data_ptr(), info.data_ptr(), B, Np, wp, nbytes, self.lib.WS_INITIALISED, st), "potrf_ws")
        else:
            assert self.entry == "plain"
            self.lib.check(L.volt_potrf_f32(A.data_ptr(), W.data_ptr(), info.data_ptr(), B, Np, st), "potrf")
        return torch.tril(A), W, info

    def lref(self, b, kind):
        return pc.clean_factor(self.B, self.N, b)[0] if kind == "schur" else None


def _check_left_behind(run, res, b, i, what):
    """(e) what a failed series' outputs hold."""
    if run.entry == "mll":
        assert bool(torch.isnan(res[0][b, 0])), (what, "out[b,0] of a failed series", float(res[0][b, 0]))
        if run.wg:
            assert bool(torch.isnan(res[1][b]).all()), (what, "alpha[b] of a failed series")
        else:
            assert bool((res[1][b] == SENTINEL).all()), (what, "alpha is not written without the gradient")
    else:
        assert bool(torch.isnan(res[0][b, i, i])), (what, "L[i,i] of the failed pivot", float(res[0][b, i, i]))


@pytest.mark.parametrize("name", list(pc.PATHS))
def test_first_failed_pivot_on_every_path(ops, schedules, name):
    _check_path(ops, name, schedules[name])


def _check_path(ops, name, schedule):
    run = _Runner(ops, name)
    B, N = run.B, run.N
    clean = run.run(run.K)
    assert clean[-1].cpu().tolist() == [0] * B, (name, "clean", clean[-1].cpu().tolist())
    calls = pc.calls(B, N, run.full)
    ncases = 0
    run.slowest = 0.0                                        # (the first call of a process loads the code objects: not counted)
    for call in calls:
        plants = [(b, pc.plant(run.Kh[b], run.sh[b], i, kind, run.lref(b, kind)), [i]) for b, i, kind in call]
        res = run.run(run.planted(plants))
        want = [0] * B
        for b, i, _kind in call:
            want[b] = i + 1
        info = res[-1].cpu().tolist()
        assert info == want, (name, call, info)                                   # (a)
        keep = torch.tensor([b for b in range(B) if want[b] == 0], device="cuda", dtype=torch.long)
        if len(keep):                                                             # (b): bit for bit (every path sums in a fixed order)
            for x, x0 in zip(res[:-1], clean[:-1]):
                assert torch.equal(x[keep], x0[keep]), (name, call, "a clean series moved")
        for b, i, _kind in call:
            _check_left_behind(run, res, b, i, (name, call))                      # (e)
        ncases += len(call)
    b = B // 2
    for pair in pc.doubles(N):                                                    # (d)
        Kp = pc.plant_double(run.Kh[b], run.sh[b], pair, pc.clean_factor(B, N, b)[0])
        res = run.run(run.planted([(b, Kp, [pair[0][0], pair[1][0]])]))
        want = [0] * B
        want[b] = pair[0][0] + 1
        assert res[-1].cpu().tolist() == want, (name, pair, res[-1].cpu().tolist())
        _check_left_behind(run, res, b, pair[0][0], (name, pair))
    assert run.slowest < HALF_A_TIMEOUT, (name, f"a call with a failed series took {run.slowest:.2f} s")   # (f)
    again = run.run(run.K)                                                        # (c)
    assert again[-1].cpu().tolist() == [0] * B, (name, "clean again", again[-1].cpu().tolist())
    for x, x0 in zip(again[:-1], clean[:-1]):
        assert torch.equal(x, x0), (name, "the clean batch after the failing calls")
    print(f"path {name} [{schedule}]: {ncases} (i, kind) cases in {len(calls)} calls, {len(pc.doubles(N))} double failures; "
          f"slowest failing call {1e3 * run.slowest:.1f} ms")


def _balanced_schedule_is_what_the_shape_gets(ops, B, N):
    """The gate of chol.hip (run_factor_groups, sched_build) restated for the factorisation alone with the batched one launch
    off: scratch with a table region, 3 .. 64 matrices, n > kmin + 1 block columns from 8 matrices on, kmin = 12 below 48
    matrices per 256 slots; and the piece list of a scheduled column has cut tiles.  Host only: which kernel a launch ran is not
    something the device is asked here, so the path keeps its launch-per-column name."""
    from volt_amd import _lib
    L = _lib.lib()
    n = ops.padded_n(N) // 128
    topo = (ctypes.c_int * 7)()
    L.volt_topology_describe(topo)
    assert list(topo)[:3] == [256, 8, 256] and not topo[6] & 4, list(topo)       # the full chip, the batched one launch off
    assert L.volt_potrf_workspace_bytes(B, ops.padded_n(N)) > 0
    kmin = 12
    assert 8 <= B < 10 and n > kmin + 1 and n >= 8                                # (one stream group, one table)
    items = (ctypes.c_int * (4 * 4096))()
    cnt = L.volt_sched_describe(B, n, 0, kmin, 256, 4, 0.6, items, 4096, None)
    assert cnt > 0
    slices = {(items[4 * x + 2] >> 8) & 255 for x in range(cnt)}
    assert max(slices) > 1, slices
    return f"columns (balanced tables from block column {kmin} of {n}: {cnt} pieces in its launch, tiles in up to {max(slices)} K-slices; gate restated on the host)"


def _child(name):
    """`python tests/test_gpu_failed_pivot.py NAME` in a process started with the path's environment."""
    from volt_amd import ops
    _entry, B, N, _opt, _sched, _full, _env = pc.TUNED_PATHS[name]
    schedule = _balanced_schedule_is_what_the_shape_gets(ops, B, N)
    print(f"path {name}: potrf ({B}, {N}) -> {schedule}")
    _check_path(ops, name, schedule)


@pytest.mark.parametrize("name", list(pc.TUNED_PATHS))
def test_first_failed_pivot_on_a_schedule_only_a_tuned_process_reaches(name):
    """The balanced table schedule of the launch-per-column factorisation: the same checks, in a child process whose environment
    switches the batched one launch off (pivot_cases.TUNED_PATHS says why it takes one)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("VOLT_")}
    env.update(pc.TUNED_PATHS[name][6], PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), name], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    assert f"path {name} [columns (balanced tables" in out.stdout


if __name__ == "__main__":
    _child(sys.argv[1])

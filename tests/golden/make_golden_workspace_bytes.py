"""Record what the library's workspace-size queries answer, over a grid of shapes, into workspace_bytes.json.  No GPU.

    python tests/golden/make_golden_workspace_bytes.py            # rewrites tests/golden/workspace_bytes.json

The sizes are part of the C ABI (callers allocate by them, and the regions inside are carved from the same sums), so a change
of the host code that is meant to leave the layouts alone is held against this table (tests/test_workspace_layout_host.py).
Two tables: the full chip (256 CUs in 8 XCDs -- what a process without a device assumes), and a faked 64-CU / 2-XCD device
(VOLT_TUNE=1 VOLT_FAKE_CUS=64 VOLT_FAKE_XCCS=2), where the topology guard switches the one-launch steps off.  The knobs are
read once per process, so each table is collected in a child process of its own (`--collect`)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_bytes.json")

BS = (1, 2, 3, 7, 8, 9, 10, 16, 24, 31, 32, 40, 64, 65, 96)
NS = (100, 128, 256, 399, 1000, 1024, 1536, 2048, 3072, 4096)
GRADS = (0, 1)
TASKS = (1, 4, 64)
CV_KCS = (1, 8)
BM_KCS = (0, 3)
TOPOLOGIES = {"full_chip": {}, "fake_64cu_2xcd": {"VOLT_TUNE": "1", "VOLT_FAKE_CUS": "64", "VOLT_FAKE_XCCS": "2"}}


def collect():
    """{query: nested lists in grid order}: [B][N][want_grad] for the three-argument queries, [B][N] for the (B, Np)
    ones (asked with the padded size), [N][T][want_dk] for the multi-task GPCV step, [B][N][want_dk][Kc] for the "cv" GPCV
    step and [B][N][Kc] for the Brownian-motion one."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from volt_amd import _lib
    L = _lib.lib()
    t = {}
    for q in ("volt_mll_workspace_bytes", "volt_mll_workspace_bytes_f64", "volt_gpcv_workspace_bytes"):
        t[q] = [[[int(getattr(L, q)(B, N, g)) for g in GRADS] for N in NS] for B in BS]
    for q in ("volt_potrf_workspace_bytes", "volt_potrf_workspace_bytes_f64", "volt_trtri_workspace_bytes_f64"):
        t[q] = [[int(getattr(L, q)(B, L.volt_padded_n(N))) for N in NS] for B in BS]
    t["volt_gpcv_mt_workspace_bytes"] = [[[int(L.volt_gpcv_mt_workspace_bytes(N, T, g)) for g in GRADS] for T in TASKS] for N in NS]
    t["volt_gpcv_cv_workspace_bytes"] = [[[[int(L.volt_gpcv_cv_workspace_bytes(B, N, g, k)) for k in CV_KCS] for g in GRADS] for N in NS] for B in BS]
    t["volt_gpcv_bm_workspace_bytes"] = [[[int(L.volt_gpcv_bm_workspace_bytes(B, N, k)) for k in BM_KCS] for N in NS] for B in BS]
    return t


def collect_in_child(topology):
    env = dict(os.environ)
    for k in ("VOLT_TUNE", "VOLT_FAKE_CUS", "VOLT_FAKE_XCCS"):
        env.pop(k, None)
    env.update(TOPOLOGIES[topology])
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--collect"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-800:])
    return json.loads(out.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    if "--collect" in sys.argv:
        print(json.dumps(collect()))
    else:
        table = {"grid": {"B": BS, "N": NS, "want_grad": GRADS, "T": TASKS, "Kc_cv": CV_KCS, "Kc_bm": BM_KCS}}
        table.update({name: collect_in_child(name) for name in TOPOLOGIES})
        with open(OUT, "w") as fh:
            json.dump(table, fh, separators=(",", ":"))
            fh.write("\n")
        print(OUT)

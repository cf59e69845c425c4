"""Outputs of volt_gpcv_step_f32 from ANY build of the library, for comparing two builds bit for bit (e.g. the parent
commit's libvolt_hip.so against this tree's after a change that must leave the "exp" step alone).

    python scripts/gpcv_step_dump.py dump  PATH/TO/libvolt_hip.so OUT.pt     # raw ctypes: no source-hash check
    python scripts/gpcv_step_dump.py compare A.pt B.pt                        # exit status 1 unless every tensor is equal

Shapes (B x N) 1 x 200, 3 x 399, 9 x 640 with grad_K; inputs are the recipe of tests/test_gpu_gpcv.py::_problem."""
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
SHAPES = ((200, 1), (399, 3), (640, 9))
NAMES = ("out", "grad_m", "grad_mu", "grad_Lq", "grad_K", "info")


def dump(path, out_path):
    from oracle import gpcv_oracle as GO
    from test_gpu_gpcv import _problem
    from volt_amd import _lib
    L = C.CDLL(path)
    for name in ("volt_gpcv_workspace_bytes", "volt_gpcv_step_f32", "volt_mll_workspace_init_f32"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib._SIGS[name]
    dev = "cuda:0"
    res = {}
    for n, B in SHAPES:
        probs = [_problem(n, 2019 + b) for b in range(B)]
        f32 = lambda ts: torch.stack([t.to(torch.float32) for t in ts]).to(dev).contiguous()
        K = f32([GO.bm_cov(probs[0][0], torch.tensor(0.2, dtype=torch.float64))] * B)
        m, Lq, y = f32([p[2] for p in probs]), f32([p[3] for p in probs]), f32([p[1] for p in probs])
        r = (m - f32([p[4].expand(n) for p in probs])).contiguous()
        gx, gw = GO.gauss_hermite(75)
        gx, gw = gx.float().to(dev), (gw / math.sqrt(math.pi)).float().to(dev)
        buf = torch.empty(L.volt_gpcv_workspace_bytes(B, n, 1) + 256, dtype=torch.uint8, device=dev)
        ptr = (buf.data_ptr() + 255) // 256 * 256
        s = torch.cuda.current_stream().cuda_stream
        assert L.volt_mll_workspace_init_f32(ptr, B, n, 1, s) == 0
        f = dict(dtype=torch.float32, device=dev)
        o = [torch.empty(B, 12, **f), torch.empty(B, n, **f), torch.empty(B, n, **f), torch.empty(B, n, n, **f),
             torch.empty(B, n, n, **f), torch.empty(B, dtype=torch.int32, device=dev)]
        rc = L.volt_gpcv_step_f32(K.data_ptr(), n, n * n, 1e-3, r.data_ptr(), m.data_ptr(), Lq.data_ptr(), y.data_ptr(),
                                  gx.data_ptr(), gw.data_ptr(), 75, 1e-6, 1e-3, 1.0 / n, 1.0 / n, *[t.data_ptr() for t in o],
                                  ptr, B, n, 2, s)
        torch.cuda.synchronize()
        assert rc == 0 and int(o[5].abs().sum()) == 0, (rc, o[5])
        res[f"{B}x{n}"] = {k: t.cpu() for k, t in zip(NAMES, o)}
    torch.save(res, out_path)
    print("dumped", path, "->", out_path, {k: float(v["out"][0, 9]) for k, v in res.items()})


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    same = True
    for shape in a:
        for k in NAMES:
            eq = torch.equal(a[shape][k], b[shape][k])
            same &= eq
            print(shape, k, "identical" if eq else "DIFFERENT")
    print("ALL IDENTICAL" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)

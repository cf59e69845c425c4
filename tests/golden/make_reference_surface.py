#!/usr/bin/env python3
"""Record the reference's public surface as names only (reference_surface.json), for the CPU tests that pin ours to it.

The reference's files are parsed with ``ast``, never imported or copied: what is written is lists of names, argument
names and literal defaults --
  * gpytorch_attrs   every ``gpytorch.<sub>.<attr>`` that train_utils.py / rollout_utils.py look up;
  * functions        every top-level function of those two files: argument names in order and literal defaults
                     ("?" where a default is not a literal);
  * classes          for each class of the reference's model / mean / kernel / likelihood files: its public methods
                     and the constructor's argument names after ``self``;
  * driver_imports   every ``from voltron... / gpytorch... import`` name of the stock and weather drivers (the
                     network download helpers under voltron.data are out of scope and left out).

Usage:  python tests/golden/make_reference_surface.py <reference checkout>
"""
import ast
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_surface.json")
CLASSES = {"models/VoltMagpie.py": ["VoltMagpie"], "models/VoltronGP.py": ["VoltronGP"], "models/Volt.py": ["Volt"],
           "models/BMGP.py": ["BMGP"],
           "models/single_task_variational_gp.py": ["SingleTaskVariationalGP"],
           "means/EWMA.py": ["EWMAMean", "DEWMAMean", "TEWMAMean", "MeanRevertingEMAMean"],
           "means/loglinear_mean.py": ["LogLinearMean"], "kernels/VolKernel.py": ["VolatilityKernel"],
           "kernels/BMKernel.py": ["BMKernel"], "kernels/FBMKernel.py": ["FBMKernel"],
           "likelihoods/volatility_likelihood.py": ["VolatilityGaussianLikelihood"]}
DRIVERS = ("stocks/GenerateMultiMeanPreds.py", "weather/GPGenerator.py", "weather/BasicWind.py")


def parse(path):
    with open(path) as fh:
        return ast.parse(fh.read())


def main(ref):
    pkg = os.path.join(ref, "voltron")
    out = {"gpytorch_attrs": {}, "functions": {}, "classes": {}, "driver_imports": {}}
    for rel in ("train_utils.py", "rollout_utils.py"):
        tree = parse(os.path.join(pkg, rel))
        names = set()
        for node in ast.walk(tree):
            if (isinstance(node, ast.Attribute) and isinstance(node.value, ast.Attribute)
                    and isinstance(node.value.value, ast.Name) and node.value.value.id == "gpytorch"):
                names.add((node.value.attr, node.attr))
        out["gpytorch_attrs"][rel] = [list(p) for p in sorted(names)]
        funcs = {}
        for node in tree.body:
            if isinstance(node, ast.FunctionDef):
                a = node.args
                defaults = [ast.literal_eval(d) if isinstance(d, (ast.Constant, ast.UnaryOp)) else "?" for d in a.defaults]
                funcs[node.name] = {"args": [x.arg for x in a.args], "defaults": defaults}
        out["functions"][rel] = funcs
    for rel, wanted in CLASSES.items():
        classes = {}
        for node in parse(os.path.join(pkg, rel)).body:
            if not (isinstance(node, ast.ClassDef) and node.name in wanted):
                continue
            fns = [f for f in node.body if isinstance(f, ast.FunctionDef)]
            init = [f for f in fns if f.name == "__init__"]
            classes[node.name] = {"methods": [f.name for f in fns if not f.name.startswith("_") or f.name == "__init__"],
                                  "init_args": [a.arg for a in init[0].args.args][1:] if init else None}
        out["classes"][rel] = classes
    for rel in DRIVERS:
        for node in ast.walk(parse(os.path.join(ref, "experiments", rel))):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in ("voltron", "gpytorch"):
                if node.module.startswith("voltron.data"):
                    continue
                out["driver_imports"].setdefault(node.module, [])
                out["driver_imports"][node.module] += [a.name for a in node.names]
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__.strip().splitlines()[-1])
    main(sys.argv[1])

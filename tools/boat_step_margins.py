"""Reference margins of the boat step's per-stage parity tests (CPU only).

    python tools/boat_step_margins.py [--native FIGURES.json] [--out profiles/r14_boat_step_margins.json]
                                      [--write-constants]

Steps every case of oracle/boat_step_cases.py once with the numpy reference
(oracle/boat_oracle.OracleVecBoat) and measures each stage against the mpmath
stages (oracle/boat_step_mp.py), each from the reference's own upstream values,
exactly as tests/test_boat_step_mp_gpu.py measures the kernel. Writes

* ``c_ref`` per config and stage -- the reference's worst error over the finite
  cases, in the stage's unit -- and ``bar = 4 c_ref``, the kernel's bar;
* the worst figure per stage and family, for reading.

``--write-constants`` also rewrites the ``C_REF`` block of
oracle/boat_step_cases.py (tests/test_boat_step_mp_cpu.py asserts that the
block and the file agree). ``--native`` merges the figures a GPU run of
tests/test_boat_step_mp_gpu.py recorded (SACENV_STEP_RECORD=<file>) as the
``native`` half of the file (the native ``obs`` figure is the float32 entry's
error over its own bar, half a float32 ulp plus the float64 bar: at most 1).
"""
import argparse
import json
import os
import pprint
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sac-agent_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

BEGIN, END = "# --- C_REF begin\n", "# --- C_REF end\n"


def reference() -> dict:
    import mpmath
    import numpy as np
    import boat_step_cases as K
    configs = {}
    for name in K.CONFIGS:
        cl = K.build(name)
        worst, fails = K.measure(cl, K.numpy_step(cl), None, obs_f32=False)
        assert not fails, fails[:5]      # the exact rules and classes hold for the reference itself
        c_ref = K.overall(worst, for_c_ref=True)
        configs[name] = {"cases": cl.N, "families": {f: int((cl.family == f).sum()) for f in sorted(set(cl.family))},
                         "c_ref": c_ref, "bar": {s: K.BAR_FACTOR * v for s, v in c_ref.items()},
                         "worst_by_family": worst}
    return {"what": "oracle/boat_oracle.OracleVecBoat against oracle/boat_step_mp.py; units there",
            "numpy": np.__version__, "mpmath": mpmath.__version__, "bits": K.M.PREC,
            "bar_factor": K.BAR_FACTOR, "configs": configs}


def write_constants(ref: dict) -> None:
    path = os.path.join(ROOT, "oracle", "boat_step_cases.py")
    with open(path) as f:
        src = f.read()
    a, b = src.index(BEGIN) + len(BEGIN), src.index(END)
    block = "C_REF = " + pprint.pformat({n: c["c_ref"] for n, c in ref["configs"].items()}, width=100,
                                        sort_dicts=False) + "\n"
    with open(path, "w") as f:
        f.write(src[:a] + block + src[b:])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_boat_step_margins.json"))
    ap.add_argument("--native", help="figures recorded by the GPU test module (merged as 'native')")
    ap.add_argument("--write-constants", action="store_true")
    args = ap.parse_args()
    doc = {"reference": reference()}
    if args.native:
        native = {}
        with open(args.native) as f:     # one JSON object per line, a later one replacing an earlier
            for line in f:
                if line.strip():
                    native.update(json.loads(line))
        doc["native"] = native
    elif os.path.exists(args.out):       # keep the native half of an earlier run
        with open(args.out) as f:
            old = json.load(f)
        if "native" in old:
            doc["native"] = old["native"]
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    if args.write_constants:
        write_constants(doc["reference"])
    for name, c in doc["reference"]["configs"].items():
        print(f"{name}: {c['cases']} cases")
        for s, v in c["c_ref"].items():
            nat = doc.get("native", {}).get(name, {}).get("worst", {}).get(s)
            print(f"  {s:7s} c_ref {v:8.3f}  bar {c['bar'][s]:8.3f}" + (f"  native {nat:8.3f}" if nat is not None else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())

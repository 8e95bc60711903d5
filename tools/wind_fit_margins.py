"""Reference margins of the wind fit's parity tests (CPU only).

    python tools/wind_fit_margins.py [--native FIGURES.json] [--out profiles/wind_fit_margins.json]
                                     [--write-constants]

Evaluates every case of oracle/wind_fit_cases.py with the numpy reference
(oracle/boat_oracle.wind_from_knots) at the case's judged indices and measures
it against the mpmath wind (oracle/wind_fit_mp.py), exactly as
tests/test_wind_fit_mp_gpu.py measures the kernel. Writes

* ``c_ref`` per config -- the reference's worst error over the decisive cases, in
  eps x top over the renormalisation's span -- and ``bar = 4 c_ref``, the kernel's
  bar at each of its two stages;
* the worst figure per family (near ties apart), the number of near ties and
  the ones the reference did not decide as the exact branch, for reading.

``--write-constants`` also rewrites the ``C_REF`` block of
oracle/wind_fit_cases.py (tests/test_wind_fit_mp_cpu.py asserts that the block
and the file agree). ``--native`` merges the figures a GPU run of
tests/test_wind_fit_mp_gpu.py recorded (SACENV_WIND_RECORD=<file>) as the
``native`` half of the file.
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
    import scipy
    import wind_fit_cases as K
    configs = {}
    for name in K.CONFIGS:
        cl = K.build(name)
        c_ref, worst = K.c_ref_of(cl)
        report: list = []
        _, fails = K.measure(cl, K.numpy_reference(cl), K.BAR_FACTOR * c_ref, is_reference=True, report=report)
        fams = [cu["family"] for _, _, cu in cl.curves()]
        configs[name] = {"experiment": cl.exp, "knots": cl.nk, "L": cl.L, "cases": cl.N, "curves": len(fams),
                         "knots_sha256": K.knots_digest(cl),
                         "families": {f: fams.count(f) for f in sorted(set(fams))},
                         "c_ref": c_ref, "bar": K.BAR_FACTOR * c_ref, "worst_by_family": worst["table"],
                         "near_ties": K.tie_summary(report), "reference_failures": [m for _, m in fails]}
    return {"what": "oracle/boat_oracle.wind_from_knots against oracle/wind_fit_mp.py; units in "
                    "oracle/wind_fit_cases.py",
            "numpy": np.__version__, "scipy": scipy.__version__, "mpmath": mpmath.__version__, "bits": K.W.PREC,
            "bar_factor": K.BAR_FACTOR, "configs": configs}


def write_constants(ref: dict) -> None:
    path = os.path.join(ROOT, "oracle", "wind_fit_cases.py")
    with open(path) as f:
        src = f.read()
    a, b = src.index(BEGIN) + len(BEGIN), src.index(END)
    block = "C_REF = " + pprint.pformat({n: c["c_ref"] for n, c in ref["configs"].items()}, width=100,
                                        sort_dicts=False) + "\n"
    with open(path, "w") as f:
        f.write(src[:a] + block + src[b:])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wind_fit_margins.json"))
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
        nat = doc.get("native", {}).get(name, {}).get("worst", {})
        print(f"{name}: {c['curves']} curves, {c['near_ties']['count']} near ties, c_ref {c['c_ref']:7.3f} "
              f"bar {c['bar']:7.3f}" + "".join(f"  native {s} {v:7.3f}" for s, v in sorted(nat.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())

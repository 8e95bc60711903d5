#!/usr/bin/env python
"""What torch CPU float32 shows against the weighted f64 oracle (tests/weighted_sac_oracle.py) on
the inputs of the weighted-learn parity tests: the ``reference`` half of
profiles/weighted_learn_f64_margins.json, from which the bar c_w = 4 x c_ref_w is taken.

    python tools/weighted_learn_margins.py [--out profiles/weighted_learn_f64_margins.json]
        [--native FILE]    # merge the figures a GPU run of tests/test_weighted_learn_gpu.py recorded
                           # (SACENV_WEIGHTED_RECORD=FILE) as the ``native`` half

Needs no GPU. An existing ``native`` half is kept unless --native replaces it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sac-agent_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_learn_f64_margins.json"))
    ap.add_argument("--native", default=None)
    a = ap.parse_args()
    import torch

    import sac_f64_cases as K
    import weighted_sac_oracle as W
    cases = {}
    for name in K.CASES:
        cases.update(W.torch_reference_weighted(name))
    c_ref_w = max(c["c_ref_max"] for c in cases.values())
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["reference"] = {
        "what": "VecSAC('cpu').learn(batch, noise, weights) in float32 against learn_f64_weighted, per tensor: "
                "max |g - g_f64| / (2^-24 S_max); losses: |L - L_f64| / (2^-24 mean |weighted row term|)",
        "torch": torch.__version__, "beta": W.BETA, "cases": cases, "c_ref_w": c_ref_w, "factor": 4,
        "c_w": W.C_W, "other_nets_max": max(c["other_max"] for c in cases.values()),
        "unweighted_bar": K.C_GRAD}
    if a.native:
        with open(a.native) as f:
            doc["native"] = json.load(f)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"c_ref_w = {c_ref_w:.3f}; 4 x = {4 * c_ref_w:.3f}; C_W = {W.C_W}")


if __name__ == "__main__":
    main()

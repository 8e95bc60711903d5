"""Reference margins of the SAC f64 parity tests (CPU only).

    python tools/sac_f64_margins.py [--native FIGURES.json] [--out profiles/r10_sac_f64_margins.json]

Runs every learn() case and act configuration of oracle/sac_f64_cases.py on
torch CPU float32 against the float64 oracle (oracle/sac_f64.py) and writes:

* ``c_ref`` per case, tensor and loss — torch's error in units of
  2^-24 S_max (gradients) or 2^-24 mean |per-row term| (losses) — and
  ``c = 4 max c_ref``, the bar of the native kernels;
* ``c_a`` / ``c_l`` the same way for the policy draw's action and log-prob;
* the Adam restatement's distance to torch's own step in ulps, and the bound
  ``max(2, 2 x that)``;
* the share of candidate rows the kink filter rejected per case (cap 25 %),
  and for the second step the share its |x| limit rejected.

``--native`` merges the figures a GPU run of tests/test_sac_native_f64_gpu.py
recorded (SACENV_F64_RECORD=<file>) as the ``native`` half of the file.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sac-agent_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def reference() -> dict:
    import torch
    import sac_f64_cases as K
    cases = {}
    for name in K.CASES:
        cases.update(K.torch_reference(name))
    act = K.torch_act_reference()
    c_ref_max = max(c["c_ref_max"] for c in cases.values())
    ulps = {q: max(max(c[w][q] for w in ("adam_ulps_own_grad", "adam_ulps_read_back")) for c in cases.values())
            for q in ("exp_avg_sq", "param", "target")}
    return {
        "what": "torch CPU float32 against oracle/sac_f64.py; units in oracle/sac_f64_cases.py",
        "torch": torch.__version__, "torch_threads": torch.get_num_threads(),
        "delta_z": K.DELTA_Z, "delta_q": K.DELTA_Q, "max_reject": K.MAX_REJECT, "x_limit_step2": K.X_LIMIT,
        "cases": cases,
        "c_ref_max": c_ref_max, "c": 4 * c_ref_max,
        "c_a_ref": act["c_a_ref"], "c_a": 4 * act["c_a_ref"],
        "c_l_ref": act["c_l_ref"], "c_l": 4 * act["c_l_ref"],
        "adam_ulps_ref": ulps, "adam_ulps_bound": {q: max(2.0, 2 * u) for q, u in ulps.items()},
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_sac_f64_margins.json"))
    ap.add_argument("--native", help="figures recorded by the GPU test module (merged as 'native')")
    args = ap.parse_args()
    doc = {"reference": reference()}
    if args.native:
        with open(args.native) as f:
            doc["native"] = json.load(f)
    elif os.path.exists(args.out):   # keep the native half of an earlier run
        with open(args.out) as f:
            old = json.load(f)
        if "native" in old:
            doc["native"] = old["native"]
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    r = doc["reference"]
    for name, c in r["cases"].items():
        print(f"{name:22s} rejected {c['rejected_share']:.3f} saturated {c['saturated_share']:.3f}  "
              f"c_ref max {c['c_ref_max']:.2f}  "
              f"adam ulps {c['adam_ulps_own_grad']} / {c['adam_ulps_read_back']}")
    print(f"c = {r['c']:.2f}  c_a = {r['c_a']:.2f}  c_l = {r['c_l']:.2f}  "
          f"adam ulps <= {r['adam_ulps_bound']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

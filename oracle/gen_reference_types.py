"""TEST INFRASTRUCTURE ONLY -- the registry TYPE names that the reference's shipped YAMLs (config/*.yaml, config_eval/*.yaml) ask for:
models, the backbone / head of the regression model, losses, metrics, datasets (run in the build container; output committed as
tests/golden/reference_yaml_types.json, read by tests/test_host_logic.py::test_every_type_named_by_the_reference_yamls_is_registered)."""
import glob
import json
import os
import sys

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402


def main():
    files = sorted(glob.glob(os.path.join(ref_import.REF_ROOT, "config", "*.yaml")) +
                   glob.glob(os.path.join(ref_import.REF_ROOT, "config_eval", "*.yaml")))
    if not files:
        raise SystemExit("reference tree not present")
    out = []
    for f in files:
        c = yaml.safe_load(open(f))
        rec = {"file": os.path.relpath(f, ref_import.REF_ROOT), "MODEL": [], "BACKBONE": [], "HEAD": [], "CRITERION": [], "EVALUATOR": [],
               "DATASET": []}
        for a in (c["ARCH"] if isinstance(c["ARCH"], list) else [c["ARCH"]]):
            rec["MODEL"].append(a["TYPE"])
            if a["TYPE"] == "HOPRegNet":            # its backbone / head are registry-built torch modules
                rec["BACKBONE"].append(a["BACKBONE"]["TYPE"])
                rec["HEAD"].append(a["HEAD"]["TYPE"])
        for key in ("CRITERION", "EVALUATOR"):
            rec[key] = [e["TYPE"] for e in c.get(key) or []]
        for split in ("TRAIN", "TEST"):
            d = (c.get("DATASET") or {}).get(split)
            if d:
                rec["DATASET"].append(d["TYPE"])
        out.append(rec)
    dst = os.path.join(ROOT, "tests", "golden", "reference_yaml_types.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(dst, len(out), "files")


if __name__ == "__main__":
    main()

"""Fixture for the registry test (tests/test_plugin_cpu.py) -- needs the reference checkout (oracle/refload.REF_ROOT).

  python tools/gen_golden_config.py     # rewrites tests/golden/reference_config.json

The reference's only config file (projects/configs/far3d.py), parsed by far3d_amd.config.load_config, reduced to the entries the
test checks (`model`, `point_cloud_range`) and stored as JSON.  Fixtures hold data only.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from far3d_amd import config  # noqa: E402
from oracle import refload  # noqa: E402

KEYS = ("model", "point_cloud_range")


def main():
    cfg = config.load_config(os.path.join(refload.REF_ROOT, "projects", "configs", "far3d.py"))
    out = os.path.join(ROOT, "tests", "golden", "reference_config.json")
    with open(out, "w") as f:
        json.dump({k: cfg[k] for k in KEYS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()

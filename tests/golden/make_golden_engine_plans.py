"""Generates tests/golden/engine_plans.json: the launch census (per kernel family the number of launches and the summed `work`
of one encode + one decode, from the engine's timing report) of every entry of the matrix of tests/test_gpu_engine_plan.py.
Needs the MI355X and the built library:

    python tests/golden/make_golden_engine_plans.py [OUT.json]

The file records WHICH data flow each block takes.  Regenerate it only in a change that means to alter the data flow (a new
fused stage, another tile family's call site, a retired option) and review the diff of the JSON like code: a refactoring of the
dispatch must leave it byte for byte as it is, which is what the test is for.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_gpu_engine_plan as tp  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else tp.PLANS
    models, plans = {}, {}
    for eid, name, opts, clips in tp.MATRIX:
        c = tp.golden_case(name)
        key = (c.stage, c.mode, tuple(sorted(c.overrides.items())), c.profile)
        if key not in models:
            models[key] = tp.build_model(c)
        census, _ = tp.run_entry(models[key], c, opts, clips)
        plans[eid] = census
        print(eid, {k: v["calls"] for k, v in census.items()}, flush=True)
    with open(out_path, "w") as f:
        json.dump({"format": 1, "plans": plans}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(plans)} plans to {out_path}")


if __name__ == "__main__":
    main()

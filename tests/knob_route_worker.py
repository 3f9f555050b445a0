"""Worker of tests/test_zzzzzzzzzzzz_knob_routes_gpu.py: started with the environment of ONE step of tests/knob_route_cases.py (the tuning knobs are read once, when
the library loads).  Runs the step's body (engine_step_run / ppo_step_run of the test module, which import the existing helpers of
test_zzzzzzz_vae_engine_shapes_gpu.py, test_ops_gpu.py and test_r_ppo_shapes_gpu.py) and prints its result as one JSON line behind the MEASURE lines."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    import knob_route_cases as kc
    import test_zzzzzzzzzzzz_knob_routes_gpu as tk
    s = kc.STEPS[sys.argv[1]]
    for name, value in s.env.items():                       # the child really runs under the step's knobs
        assert os.environ.get(name) == value, (name, os.environ.get(name), value)
    stray = sorted(k for k in os.environ if k.startswith("MI355_") and k not in s.env and k in {r.env for r in kc.table_rows()})
    assert not stray, stray
    print(json.dumps(tk.ppo_step_run(s) if s.kind == "ppo" else tk.engine_step_run(s)))

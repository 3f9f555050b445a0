"""Worker of test_environment_only_knobs_in_child_processes (tests/test_zzz_dense_shapes_gpu.py): one step of dense_shape_cases.ENV_STEPS, started with the step's
environment-only knobs set (they are read when the library is loaded: a process has them or has them not).  The step's cases run on the kernels the knobs leave them,
against the same float64 references and bounds.  Prints its MEASURE lines, then the list of what ran as one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    import test_zzz_dense_shapes_gpu as tz
    done = tz.knob_step(int(sys.argv[1]))
    tz.print_measurements()
    print(json.dumps(done))

"""Worker of test_workspace_guards_stay_intact (tests/test_zzzzzzz_vae_engine_shapes_gpu.py): started with MI355_DEBUG_GUARDS=1, which the engine reads when a workspace
is sized and carved.  One case of vae_engine_cases.py in all three precisions: a training step, encode, reconstruct, generate; prints the guard counts as one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    import test_zzzzzzz_vae_engine_shapes_gpu as tz
    print(json.dumps(tz.guard_run(int(sys.argv[1]))))

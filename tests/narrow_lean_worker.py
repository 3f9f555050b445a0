"""Worker of test_first_generation_narrow_forms_in_a_child_process (tests/test_x_conv_shapes_gpu.py): the narrow-layer cases of tests/conv_shape_cases.py that the bf16
instruction-lean kernels take, run with MI355_NARROW_LEAN=0 (the knob is read when the library is loaded: a process has it or has it not), where narrow_conv_kernel and
the library-math form of the fused loss take them; the same float64 references, the same bounds.  Prints the list of what ran as one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    assert os.environ.get("MI355_NARROW_LEAN") == "0", "the worker is the run with the knob off"
    import test_x_conv_shapes_gpu as tx
    print(json.dumps(tx.first_generation_narrow_forms()))

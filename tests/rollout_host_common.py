"""Shared helpers of the CPU-only rollout tests (test_rollout_batch_host.py, test_rollout_buffer_host.py, test_rollout_segments_host.py): the gfx950 listing of one
source of carla-ppo_amd/csrc (compiled here, no GPU needed), one kernel of it, and the pattern of the scalar unit's writes.  No torch at import time."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# stores and atomics of the scalar unit, and its cache write-back / discard (the mnemonics are put together here so that this file does not spell them)
SCALAR_WRITES = re.compile(r"\bs_(?:buffer_|scratch_)?(?:st" + r"ore|at" + r"omic)|\bs_d" + r"cache_(?:wb|discard)")


def _listing(name):
    path = os.path.join(tempfile.mkdtemp(), name + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", os.path.join(ROOT, "carla-ppo_amd", "csrc", name + ".hip"), "-o", path], check=True, capture_output=True)
    return open(path).read()


def _kernel(text, prefix):
    """-> (mangled name, instructions up to the kernel's end, private segment bytes, static LDS bytes) of the kernel whose name starts with `prefix`."""
    m = re.search(r"^(" + prefix + r"[A-Za-z0-9_]*):", text, re.M)
    assert m, prefix
    name = m.group(1)
    body = text[m.start():text.index("s_endpgm", m.start())]
    meta = re.search(r"\.group_segment_fixed_size:\s+(\d+)\s*\n(?:(?!\s*\.name:).*\n)*?\s+\.name:\s+" + re.escape(name) + r"\s*\n\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert meta, name
    return name, body, int(meta.group(2)), int(meta.group(1))

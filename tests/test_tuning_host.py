"""CPU-only: the tuning table (csrc/tuning.hip) seen through mi_set_tuning -- every key's default, clamp and restoration, the rejected keys, and how the
environment strings of the keyed knobs parse.  The expected values are literals recorded from the build BEFORE the table existed (the per-file globals and
getenv sites), by running this file as a script against that build: `MI355_LIB=<that build> python tests/test_tuning_host.py` prints them."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))
from mi355 import lib as milib

SET_VALUES = (0, 2, 7, 1000000, -5)
# one fresh child per case (knobs are process state, read from the environment once): for every key in argv[2], [the default, then what each of SET_VALUES became
# (read back as the next call's return value), what restoring the default gave back, the restored value]; for every key in argv[3], [return code, last error]
CHILD = ("import ctypes, json, sys\n"
         "L = ctypes.CDLL(sys.argv[1]); L.mi_last_error.restype = ctypes.c_char_p\n"
         "s, out = L.mi_set_tuning, {}\n"
         "for k in json.loads(sys.argv[2]):\n"
         "    d = s(k, %d)\n"
         "    out[str(k)] = [d] + [s(k, v) for v in %r] + [s(k, d), s(k, d)]\n"
         "for k in json.loads(sys.argv[3]):\n"
         "    out[str(k)] = [s(k, 1), L.mi_last_error().decode()]\n"
         "print(json.dumps(out))\n") % (SET_VALUES[0], SET_VALUES[1:])


def _child(keys, bad=(), **env_set):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355_")}
    env.update(env_set)
    r = subprocess.run([sys.executable, "-c", CHILD, milib.LIB_PATH, json.dumps(list(keys)), json.dumps(list(bad))], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


# key -> [default, after 0, after 2, after 7, after 1000000, after -5]; the last column of the child's row (the value after restoring the default) equals the first
KEYS = {
    0: [1, 0, 1, 1, 1, 1],
    1: [300, 0, 2, 7, 1000000, -1],
    2: [0, 0, 2, 7, 1000000, -5],
    3: [1, 0, 1, 1, 1, 1],
    4: [1, 0, 1, 1, 1, 1],
    5: [0, 0, 2, 7, 1000000, -5],
    6: [1, 0, 1, 1, 1, 1],
    7: [1, 0, 1, 1, 1, 1],
    8: [0, 0, 0, 0, 0, 0],
    9: [256, 16, 16, 16, 1000000, 16],
    10: [12, 0, 2, 7, 1000000, -5],
    11: [256, 1, 2, 7, 1000000, 1],
    12: [1, 0, 1, 1, 1, 1],
    13: [1, 0, 2, 2, 2, 0],
    14: [1, 0, 1, 1, 1, 1],
    15: [3, 0, 2, 3, 3, 0],
    16: [0, 0, 2, 7, 1000000, 0],
    17: [2, 0, 2, 7, 1000000, -5],
    18: [0, 0, 1, 1, 1, 1],
    19: [3, 0, 2, 7, 1000000, -5],
    20: [2, 0, 2, 7, 1000000, -5],
    21: [1, 0, 2, 7, 1000000, -5],
    22: [1, 0, 1, 1, 1, 1],
    23: [0, 0, 2, 7, 1000000, 0],
    24: [0, 0, 2, 0, 0, 0],
    25: [0, 0, 2, 7, 1000000, -5],
    26: [0, 0, 1, 1, 1, 1],
}
BAD = {12345: [-1, 'mi_set_tuning: unknown key'], -3: [-1, 'mi_set_tuning: unknown key'], 27: [-1, 'mi_set_tuning: unknown key']}

# (environment, key, parsed value): on/off strings by their first character, integers in and out of range, the tapconv pair
ENV_CASES = [
    ({'MI355_GEMM2': '0'}, 0, 0), ({'MI355_GEMM2': '1'}, 0, 1), ({'MI355_GEMM2': '2'}, 0, 1), ({'MI355_GEMM2': ''}, 0, 1), ({'MI355_GEMM2': '00'}, 0, 0), ({'MI355_GEMM2': 'x'}, 0, 1),
    ({'MI355_TAPCONV_MINBLOCKS': '0'}, 1, 0), ({'MI355_TAPCONV_MINBLOCKS': '1'}, 1, 1), ({'MI355_TAPCONV_MINBLOCKS': '2'}, 1, 2), ({'MI355_TAPCONV_MINBLOCKS': '3'}, 1, 3), ({'MI355_TAPCONV_MINBLOCKS': '4'}, 1, 4),
    ({'MI355_TAPCONV_MINBLOCKS': '7'}, 1, 7), ({'MI355_TAPCONV_MINBLOCKS': '-1'}, 1, -1), ({'MI355_TAPCONV_MINBLOCKS': '-7'}, 1, -7), ({'MI355_TAPCONV_MINBLOCKS': '100'}, 1, 100),
    ({'MI355_TAPCONV_MINBLOCKS': '1000'}, 1, 1000), ({'MI355_TAPCONV_MINBLOCKS': 'x'}, 1, 0), ({'MI355_TAPCONV_MINBLOCKS': ''}, 1, 0),
    ({'MI355_TAPCONV': '0'}, 1, -1), ({'MI355_TAPCONV': '1'}, 1, 300), ({'MI355_TAPCONV': '2'}, 1, 300), ({'MI355_TAPCONV': ''}, 1, 300), ({'MI355_TAPCONV': '00'}, 1, -1), ({'MI355_TAPCONV': 'x'}, 1, 300),
    ({'MI355_TAPWGRAD': '0'}, 3, 0), ({'MI355_TAPWGRAD': '1'}, 3, 1), ({'MI355_TAPWGRAD': '2'}, 3, 1), ({'MI355_TAPWGRAD': ''}, 3, 1), ({'MI355_TAPWGRAD': '00'}, 3, 0), ({'MI355_TAPWGRAD': 'x'}, 3, 1),
    ({'MI355_NARROW': '0'}, 4, 0), ({'MI355_NARROW': '1'}, 4, 1), ({'MI355_NARROW': '2'}, 4, 1), ({'MI355_NARROW': ''}, 4, 1), ({'MI355_NARROW': '00'}, 4, 0), ({'MI355_NARROW': 'x'}, 4, 1),
    ({'MI355_DENSE_WGRAD_BLOCKS': '0'}, 11, 0), ({'MI355_DENSE_WGRAD_BLOCKS': '1'}, 11, 1), ({'MI355_DENSE_WGRAD_BLOCKS': '2'}, 11, 2), ({'MI355_DENSE_WGRAD_BLOCKS': '3'}, 11, 3),
    ({'MI355_DENSE_WGRAD_BLOCKS': '4'}, 11, 4), ({'MI355_DENSE_WGRAD_BLOCKS': '7'}, 11, 7), ({'MI355_DENSE_WGRAD_BLOCKS': '-1'}, 11, -1), ({'MI355_DENSE_WGRAD_BLOCKS': '-7'}, 11, -7),
    ({'MI355_DENSE_WGRAD_BLOCKS': '100'}, 11, 100), ({'MI355_DENSE_WGRAD_BLOCKS': '1000'}, 11, 1000), ({'MI355_DENSE_WGRAD_BLOCKS': 'x'}, 11, 0), ({'MI355_DENSE_WGRAD_BLOCKS': ''}, 11, 0),
    ({'MI355_RWCONV': '0'}, 13, 0), ({'MI355_RWCONV': '1'}, 13, 1), ({'MI355_RWCONV': '2'}, 13, 2), ({'MI355_RWCONV': '3'}, 13, 1), ({'MI355_RWCONV': '4'}, 13, 1), ({'MI355_RWCONV': '7'}, 13, 1),
    ({'MI355_RWCONV': '-1'}, 13, 1), ({'MI355_RWCONV': '-7'}, 13, 1), ({'MI355_RWCONV': '100'}, 13, 1), ({'MI355_RWCONV': '1000'}, 13, 1), ({'MI355_RWCONV': 'x'}, 13, 0), ({'MI355_RWCONV': ''}, 13, 0),
    ({'MI355_RWCONV_CONV': '0'}, 15, 0), ({'MI355_RWCONV_CONV': '1'}, 15, 1), ({'MI355_RWCONV_CONV': '2'}, 15, 2), ({'MI355_RWCONV_CONV': '3'}, 15, 3), ({'MI355_RWCONV_CONV': '4'}, 15, 3),
    ({'MI355_RWCONV_CONV': '7'}, 15, 3), ({'MI355_RWCONV_CONV': '-1'}, 15, 3), ({'MI355_RWCONV_CONV': '-7'}, 15, 3), ({'MI355_RWCONV_CONV': '100'}, 15, 3), ({'MI355_RWCONV_CONV': '1000'}, 15, 3),
    ({'MI355_RWCONV_CONV': 'x'}, 15, 0), ({'MI355_RWCONV_CONV': ''}, 15, 0),
    ({'MI355_RWCONV_BLOCKS': '0'}, 16, 0), ({'MI355_RWCONV_BLOCKS': '1'}, 16, 1), ({'MI355_RWCONV_BLOCKS': '2'}, 16, 2), ({'MI355_RWCONV_BLOCKS': '3'}, 16, 3), ({'MI355_RWCONV_BLOCKS': '4'}, 16, 4),
    ({'MI355_RWCONV_BLOCKS': '7'}, 16, 7), ({'MI355_RWCONV_BLOCKS': '-1'}, 16, -1), ({'MI355_RWCONV_BLOCKS': '-7'}, 16, -7), ({'MI355_RWCONV_BLOCKS': '100'}, 16, 100), ({'MI355_RWCONV_BLOCKS': '1000'}, 16, 1000),
    ({'MI355_RWCONV_BLOCKS': 'x'}, 16, 0), ({'MI355_RWCONV_BLOCKS': ''}, 16, 0),
    ({'MI355_GEMM2_TILE': '0'}, 17, 0), ({'MI355_GEMM2_TILE': '1'}, 17, 1), ({'MI355_GEMM2_TILE': '2'}, 17, 2), ({'MI355_GEMM2_TILE': '3'}, 17, 3), ({'MI355_GEMM2_TILE': '4'}, 17, 4),
    ({'MI355_GEMM2_TILE': '7'}, 17, 7), ({'MI355_GEMM2_TILE': '-1'}, 17, -1), ({'MI355_GEMM2_TILE': '-7'}, 17, -7), ({'MI355_GEMM2_TILE': '100'}, 17, 100), ({'MI355_GEMM2_TILE': '1000'}, 17, 1000),
    ({'MI355_GEMM2_TILE': 'x'}, 17, 0), ({'MI355_GEMM2_TILE': ''}, 17, 0),
    ({'MI355_NW_DEPTH': '0'}, 19, 0), ({'MI355_NW_DEPTH': '1'}, 19, 1), ({'MI355_NW_DEPTH': '2'}, 19, 2), ({'MI355_NW_DEPTH': '3'}, 19, 3), ({'MI355_NW_DEPTH': '4'}, 19, 4), ({'MI355_NW_DEPTH': '7'}, 19, 7),
    ({'MI355_NW_DEPTH': '-1'}, 19, -1), ({'MI355_NW_DEPTH': '-7'}, 19, -7), ({'MI355_NW_DEPTH': '100'}, 19, 100), ({'MI355_NW_DEPTH': '1000'}, 19, 1000), ({'MI355_NW_DEPTH': 'x'}, 19, 0),
    ({'MI355_NW_DEPTH': ''}, 19, 0),
    ({'MI355_GEMM2_STAGES': '0'}, 20, 0), ({'MI355_GEMM2_STAGES': '1'}, 20, 1), ({'MI355_GEMM2_STAGES': '2'}, 20, 2), ({'MI355_GEMM2_STAGES': '3'}, 20, 3), ({'MI355_GEMM2_STAGES': '4'}, 20, 4),
    ({'MI355_GEMM2_STAGES': '7'}, 20, 7), ({'MI355_GEMM2_STAGES': '-1'}, 20, -1), ({'MI355_GEMM2_STAGES': '-7'}, 20, -7), ({'MI355_GEMM2_STAGES': '100'}, 20, 100), ({'MI355_GEMM2_STAGES': '1000'}, 20, 1000),
    ({'MI355_GEMM2_STAGES': 'x'}, 20, 0), ({'MI355_GEMM2_STAGES': ''}, 20, 0),
    ({'MI355_X3_TAPWGRAD': '0'}, 21, 0), ({'MI355_X3_TAPWGRAD': '1'}, 21, 1), ({'MI355_X3_TAPWGRAD': '2'}, 21, 2), ({'MI355_X3_TAPWGRAD': '3'}, 21, 3), ({'MI355_X3_TAPWGRAD': '4'}, 21, 4),
    ({'MI355_X3_TAPWGRAD': '7'}, 21, 7), ({'MI355_X3_TAPWGRAD': '-1'}, 21, -1), ({'MI355_X3_TAPWGRAD': '-7'}, 21, -7), ({'MI355_X3_TAPWGRAD': '100'}, 21, 100), ({'MI355_X3_TAPWGRAD': '1000'}, 21, 1000),
    ({'MI355_X3_TAPWGRAD': 'x'}, 21, 0), ({'MI355_X3_TAPWGRAD': ''}, 21, 0),
    ({'MI355_DWGS': '0'}, 22, 0), ({'MI355_DWGS': '1'}, 22, 1), ({'MI355_DWGS': '2'}, 22, 1), ({'MI355_DWGS': ''}, 22, 1), ({'MI355_DWGS': '00'}, 22, 0), ({'MI355_DWGS': 'x'}, 22, 1),
    ({'MI355_TW_LDEC': '0'}, 24, 0), ({'MI355_TW_LDEC': '1'}, 24, 1), ({'MI355_TW_LDEC': '2'}, 24, 2), ({'MI355_TW_LDEC': '3'}, 24, 3), ({'MI355_TW_LDEC': '4'}, 24, 0), ({'MI355_TW_LDEC': '7'}, 24, 0),
    ({'MI355_TW_LDEC': '-1'}, 24, 0), ({'MI355_TW_LDEC': '-7'}, 24, 0), ({'MI355_TW_LDEC': '100'}, 24, 0), ({'MI355_TW_LDEC': '1000'}, 24, 0), ({'MI355_TW_LDEC': 'x'}, 24, 0),
    ({'MI355_TW_LDEC': ''}, 24, 0),
    ({'MI355_DECTAIL_SPLIT5': '0'}, 26, 0), ({'MI355_DECTAIL_SPLIT5': '1'}, 26, 1), ({'MI355_DECTAIL_SPLIT5': '2'}, 26, 0), ({'MI355_DECTAIL_SPLIT5': ''}, 26, 0), ({'MI355_DECTAIL_SPLIT5': '10'}, 26, 1),
    ({'MI355_DECTAIL_SPLIT5': 'x'}, 26, 0),
    ({'MI355_TAPCONV': '0', 'MI355_TAPCONV_MINBLOCKS': '50'}, 1, -1), ({'MI355_TAPCONV': '1', 'MI355_TAPCONV_MINBLOCKS': '50'}, 1, 50), ({'MI355_TAPCONV': '0', 'MI355_TAPCONV_MINBLOCKS': '-4'}, 1, -1),
    ({'MI355_TAPCONV': '', 'MI355_TAPCONV_MINBLOCKS': '0'}, 1, 0),
]


def _env_cases_for(name, key, kind):
    vals = {"on": ("0", "1", "2", "", "00", "x"), "off": ("0", "1", "2", "", "10", "x"), "int": ("0", "1", "2", "3", "4", "7", "-1", "-7", "100", "1000", "x", "")}[kind]
    return [({name: v}, key) for v in vals]


ENV_KNOBS = [("MI355_GEMM2", 0, "on"), ("MI355_TAPCONV_MINBLOCKS", 1, "int"), ("MI355_TAPCONV", 1, "on"), ("MI355_TAPWGRAD", 3, "on"), ("MI355_NARROW", 4, "on"),
             ("MI355_DENSE_WGRAD_BLOCKS", 11, "int"), ("MI355_RWCONV", 13, "int"), ("MI355_RWCONV_CONV", 15, "int"), ("MI355_RWCONV_BLOCKS", 16, "int"),
             ("MI355_GEMM2_TILE", 17, "int"), ("MI355_NW_DEPTH", 19, "int"), ("MI355_GEMM2_STAGES", 20, "int"), ("MI355_X3_TAPWGRAD", 21, "int"),
             ("MI355_DWGS", 22, "on"), ("MI355_TW_LDEC", 24, "int"), ("MI355_DECTAIL_SPLIT5", 26, "off")]
PAIR_CASES = [({"MI355_TAPCONV": "0", "MI355_TAPCONV_MINBLOCKS": "50"}, 1), ({"MI355_TAPCONV": "1", "MI355_TAPCONV_MINBLOCKS": "50"}, 1),
              ({"MI355_TAPCONV": "0", "MI355_TAPCONV_MINBLOCKS": "-4"}, 1), ({"MI355_TAPCONV": "", "MI355_TAPCONV_MINBLOCKS": "0"}, 1)]


def _all_env_cases():
    return [c for name, key, kind in ENV_KNOBS for c in _env_cases_for(name, key, kind)] + PAIR_CASES


def test_every_key_has_its_default_clamp_and_restoration():
    got = _child(range(27), bad=(12345, -3, 27))
    for k, want in KEYS.items():
        row = got[str(k)]
        assert row[:-1] == want, (k, row, want)
        assert row[-1] == row[0], (k, row)
    assert set(KEYS) == set(range(27))
    for k, want in BAD.items():
        assert got[str(k)] == want, (k, got[str(k)], want)
    assert set(BAD) == {12345, -3, 27}


def test_environment_strings_of_the_keyed_knobs_parse_as_before():
    want = {(tuple(sorted(e.items())), k): v for e, k, v in ENV_CASES}
    cases = _all_env_cases()
    assert {(tuple(sorted(e.items())), k) for e, k in cases} == set(want)
    for e, k in cases:
        assert _child([k], **e)[str(k)][0] == want[(tuple(sorted(e.items())), k)], (e, k)


def test_every_environment_name_of_the_table_is_listed_in_design_section_7():
    names = set(re.findall(r"MI355_[A-Z0-9_]+", open(os.path.join(ROOT, "carla-ppo_amd", "csrc", "tuning.hip")).read()))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("\n## 7"):]
    sec = sec[:sec.index("\n## ", 1)] if "\n## " in sec[1:] else sec
    assert len(names) >= 45
    missing = sorted(n for n in names if not re.search(n + r"(?![A-Z0-9_])", sec))
    assert not missing, missing


if __name__ == "__main__":                                # record the expectations from the library MI355_LIB names
    got = _child(range(27), bad=(12345, -3, 27))
    print("KEYS = {")
    for k in range(27):
        print("    %d: %r," % (k, got[str(k)][:-1]))
    print("}\nBAD = {%s}" % ", ".join("%d: %r" % (k, got[str(k)]) for k in (12345, -3, 27)))
    print("ENV_CASES = [")
    for e, k in _all_env_cases():
        print("    (%r, %d, %d)," % (e, k, _child([k], **e)[str(k)][0]))
    print("]")

"""The measurement switches (TIP_* environment variables of the -DTIP_MEASURE build) are ONE list: the table csrc/tip_measure.h, the
comment of include/tip_hip_debug.h, the string literals of csrc/ and what the scripts under tools/ set must name the same variables,
the table has one reader, and a retired switch is named nowhere but in the history (CHANGELOG.md, docs/).  No GPU, no library."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "transformer-inertial-poser_amd", "csrc")
NAME = r"TIP_[A-Z0-9_]+"

# retired with the code only they reached (CHANGELOG.md, "one table for the measurement switches"); TIP_S16_TRACE was a name only
RETIRED = """TIP_FUSED_ABLATE TIP_TRAIN_FWD_PADDED TIP_TGEMM16_TILE TIP_TGEMM_TILE TIP_GENERAL_GEMM TIP_GENERAL_ATTN TIP_GENERAL_PGEMM
TIP_TRAIN_PGEMM TIP_TRAIN_FUSED TIP_TRAIN_FUSED_BWD TIP_TRAIN_WIN_GEMM TIP_DW_KERNEL TIP_DW_SPLITS TIP_DW_SPLITDIV TIP_DW_NB
TIP_RNN_HANDOFF TIP_RNN_PREPOLL TIP_RNN_ROTATE TIP_RNN_C16 TIP_RNN_GEMV_NM TIP_S16_TRACE""".split()

# what a script may set or show that is no switch of the library: the Python-side library choice, one script's own variable, and the
# header's constants
NOT_A_SWITCH = re.compile(r"TIP_(LIB|PLAN_BASE|OPT_\w+|PLAN_\w+|ERR_\w+|SAVED_\w+|STREAM_\w+)$")


def read(path):
    with open(path, errors="replace") as f:
        return f.read()


def csrc_sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def table_names():
    names = re.findall(r'^TIP_SWITCH\("(%s)"' % NAME, read(os.path.join(CSRC, "tip_measure.h")), re.M)
    assert len(names) == len(set(names)) and names, names
    return set(names)


def test_table_header_and_sources_name_the_same_switches():
    table = table_names()
    header = read(os.path.join(ROOT, "include", "tip_hip_debug.h"))
    comment = header[:header.index("#ifndef TIP_HIP_DEBUG_H")]
    listed = set(re.findall(NAME, comment)) - {"TIP_MEASURE"}
    assert listed == table, (sorted(listed - table), sorted(table - listed))
    literals = set()
    for f in csrc_sources():
        literals |= set(re.findall(r'"(%s)"' % NAME, read(f)))
    assert literals == table, (sorted(literals - table), sorted(table - literals))


def test_the_table_has_one_reader():
    """tip_env( occurs where it is defined (tip_internal.h) and where measure_switches() expands the table (tip_schedule.hip); the
    mentions in tip_internal.h's comments aside, nowhere else: every launcher asks measure_switches().field."""
    calls = {}
    for f in csrc_sources():
        code = re.sub(r"//[^\n]*", "", read(f))
        n = len(re.findall(r"\btip_env\s*\(", code))
        if n:
            calls[os.path.basename(f)] = n
    assert calls == {"tip_internal.h": 1, "tip_schedule.hip": 1}, calls
    sched = read(os.path.join(CSRC, "tip_schedule.hip"))
    assert re.search(r"#define TIP_SWITCH\([^)]*\)[^\n]*tip_env\(env\)[^\n]*\n#include \"tip_measure.h\"", sched)


def test_every_switch_a_tool_sets_is_in_the_table():
    table = table_names()
    unknown = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "tools")):
        for fn in files:
            if not fn.endswith((".py", ".sh", ".md")):
                continue
            text = read(os.path.join(dirpath, fn))
            used = set(re.findall(r"\b(%s)=" % NAME, text))                                  # VAR=value in a command or usage line
            used |= set(re.findall(r'environ[^\n]*?"(%s)"' % NAME, text))                    # os.environ[...] / .get / .setdefault
            for name in sorted(used):
                if name not in table and not NOT_A_SWITCH.match(name):
                    unknown.append((os.path.relpath(os.path.join(dirpath, fn), ROOT), name))
    assert not unknown, unknown


def test_no_retired_switch_outside_the_history():
    assert not set(RETIRED) & table_names()
    pat = re.compile(r"\b(%s)\b" % "|".join(RETIRED))
    # the project's own directories (docs/ is history), and the files at the top
    trees = ("examples", "include", "oracle", "profiles", "tests", "tools", "transformer-inertial-poser_amd")
    skip_dirs = {"__pycache__", "_ref", ".pytest_cache"}
    text_ext = (".py", ".sh", ".md", ".h", ".hip", ".c", ".cpp", ".txt", ".json", ".map", ".cfg", ".toml", ".ini", "Makefile")
    me = os.path.abspath(__file__)
    hits = []
    for dirpath, dirs, files in os.walk(ROOT):
        dirs[:] = [d for d in dirs if d not in skip_dirs and (dirpath != ROOT or d in trees)]
        for fn in files:
            path = os.path.join(dirpath, fn)
            if not fn.endswith(text_ext) or os.path.abspath(path) == me or os.path.relpath(path, ROOT) == "CHANGELOG.md":
                continue
            found = sorted(set(pat.findall(read(path))))
            if found:
                hits.append((os.path.relpath(path, ROOT), found))
    assert not hits, hits

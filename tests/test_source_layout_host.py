"""The layout of csrc/ as text: build.sh's one list of translation units, the include graph under them, and what a header may
hold.  No GPU, no library."""
import os
import re

from support import CSRC, ROOT, build_units

INCLUDE = re.compile(r'(?m)^\s*#\s*include\s+"([^"]+)"')


def code(name):
    """csrc/<name> without its comments"""
    text = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"(?s)/\*.*?\*/", "", text))


def reachable(src):
    """every file of csrc/ that compiling csrc/<src> reads, through .hip files and headers alike"""
    seen, todo = set(), [src]
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        todo += [inc for inc in INCLUDE.findall(code(name)) if os.path.exists(os.path.join(CSRC, inc)) and "/" not in inc]
    return seen


def test_the_units_of_build_sh_exist_and_are_listed_once():
    units = build_units()
    assert len(units) >= 8
    for unit, src in units.items():
        assert os.path.exists(os.path.join(CSRC, src)), (unit, src)
    build = re.sub(r"(?m)^\s*#.*$", "", open(os.path.join(ROOT, "build.sh")).read())
    assert "$OBJECTS -o $OUT" in build and "for tu in $UNITS" in build


def test_every_hip_file_is_a_unit_or_compiled_into_exactly_one():
    sources = sorted(set(build_units().values()))
    reach = {src: reachable(src) for src in sources}
    for name in sorted(f for f in os.listdir(CSRC) if f.endswith(".hip")):
        owners = [src for src in sources if name in reach[src]]
        if name in sources:
            assert owners == [name], (name, owners)          # a unit is no other unit's include
        else:
            assert len(owners) == 1, (name, owners)


def test_no_header_defines_a_kernel_that_is_not_a_template():
    headers = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))
    assert "dff_frames.h" in headers and "dff_analysis_host.h" in headers
    for name in headers:
        text = code(name)
        for m in re.finditer(r"__global__", text):
            head = re.split(r"[;}]", text[:m.start()])[-1]      # the declaration so far
            assert re.search(r"\btemplate\s*<", head), (name, text[m.start():m.start() + 120])


def test_the_experiment_harness_takes_its_objects_from_build_sh():
    text = open(os.path.join(ROOT, "tools_exp.sh")).read()
    assert "dff_analysis" not in text
    assert "./build.sh --objects" in text
    for unit in build_units():
        if unit not in ("dff_kernels", "dff_host") and not unit.startswith("dff_small"):   # the units an experiment rebuilds
            assert unit not in text, unit

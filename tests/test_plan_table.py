"""The step planner's decisions as a table ("Step planner: one form per plan"): tests/golden/plan_table.txt holds, for cases
on both sides of every line the planner draws, what the library does -- the launcher and its arguments, the plan-derived argument words, the scratch size,
nb_diag_plan's string, nb_diag_step_clock's verdict, the two-phase plan.  It was recorded from the planner as it stood before the
planner moved into nenbody_amd/csrc/nb_plan.h, so the header is held to the decisions of the code it replaced.

Two checks: tests/cpp/plan_table.cpp -- the header alone, no library, no HIP -- prints the table again, line for line; and the built
library, without a device, gives the table's nb_diag_plan / nb_scratch_bytes / nb_scratch_bytes_phased columns."""
import ctypes
import os
import struct
import subprocess

from conftest import GOLDEN_DIR, ROOT
from nenbody_amd import _lib

TABLE = os.path.join(GOLDEN_DIR, "plan_table.txt")
EXE = os.path.join(ROOT, "build", "plan_table")


def test_the_header_alone_prints_the_table():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "plan_table.cpp"), "-o", EXE], check=True)
    r = subprocess.run([EXE, TABLE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(TABLE) as f:
        want = f.read().splitlines()
    got = r.stdout.splitlines()
    assert len(want) > 400 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def parse(line):
    """(params, n, count, (j_lo, j_hi) or None, knobs, results of the step, results of the phases or None)"""
    case, results = line.split(" => ")
    kv = [t.split("=", 1) for t in case.split()]
    d = {k: v for k, v in kv if not k.startswith("NB_")}
    knobs = {k: v for k, v in kv if k.startswith("NB_")}
    f32 = lambda h: struct.unpack("<f", struct.pack("<I", int(h, 16)))[0]
    p = _lib.NbParams(0.1, f32(d["G"]), f32(d["bias"]), int(d["tile"]), int(d["mode"]))
    step, _, phase = results.partition(" | phase ")
    return p, int(d["n"]), int(d["count"]), ((int(d["jlo"]), int(d["jhi"])) if "jlo" in d else None), knobs, step, (phase or None)


def column(results, name):
    return next(t.split("=", 1)[1] for t in results.split() if t.startswith(name + "="))


def check_line(lib, line):
    p, n, count, phase_range, _, step, phase = parse(line)
    rc = int(column(step, "rc"))
    buf = ctypes.create_string_buffer(256)
    assert lib.nb_diag_plan(ctypes.byref(p), n, count, buf, len(buf)) == rc, line
    if rc == _lib.NB_OK:
        assert buf.value.decode() == column(step, "plan"), line
        assert lib.nb_scratch_bytes(ctypes.byref(p), n, count) == int(column(step, "scratch")), line
    else:
        assert _lib.last_error() == step.split('err="', 1)[1][:-1], line
        assert lib.nb_scratch_bytes(ctypes.byref(p), n, count) == 0, line
    if phase_range is not None:
        want = int(column(phase, "scratch")) if int(column(phase, "rc")) == _lib.NB_OK else 0
        assert lib.nb_scratch_bytes_phased(ctypes.byref(p), n, count, *phase_range) == want, line


def test_the_library_gives_the_tables_plans_and_scratch_sizes(nb, monkeypatch):
    with open(TABLE) as f:
        lines = f.read().splitlines()
    plain = [ln for ln in lines if " NB_" not in ln.split(" => ")[0]]
    knobbed = [ln for ln in lines if " NB_" in ln.split(" => ")[0]]
    assert len(plain) > 150 and len(knobbed) > 250
    for k in [k for k in os.environ if k.startswith("NB_") and k != "NB_ROCTX"]:
        monkeypatch.delenv(k)
    for ln in plain:
        check_line(_lib.load(), ln)
    for ln in knobbed[::7]:   # a few dozen, every knob's family among them
        knobs = parse(ln)[4]
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)     # (the library reads its overrides again; a legacy form's knob binds the library that holds every form)
        check_line(_lib.load(), ln)
        for k in knobs:
            monkeypatch.delenv(k)

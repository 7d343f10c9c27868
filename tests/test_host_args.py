"""csrc/host_args.h -- what every layer family's host entry point judges about a call's arrays -- held to its
definitions on the host: tests/native/host_args_host.cpp includes the header alone and sweeps spans_meet against "the byte
sets intersect", the two list policies (outputs_overlap, arrays_overlap) against their one-sentence definitions over every
list of up to four spans, csrc/solver.hip's sorted-neighbours form against "any two meet", and outputs_alias against the
O(n^2) definition.  No GPU: the refusals themselves are pinned through the library by tests/test_abi_*.py; this is the
rule they all call, and the proof that the sweep would see it change: the same program built against a copy of the header
with one rule altered reports that rule and nothing else."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mms_answer_selection_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "native", "host_args_host.cpp")

# name -> (the header's text, what it becomes, the rule the program must name)
MUTATIONS = {
    "touching spans meet": ("a.lo < b.hi && b.lo < a.hi", "a.lo <= b.hi && b.lo < a.hi", "spans_meet"),
    "an empty span meets": ("return a.lo != a.hi && b.lo != b.hi && ", "return b.lo != b.hi && ", "spans_meet"),
    "a NULL output aliases": ("    if (!outputs[i]) continue;\n", "", "outputs_alias"),
    "in place for the wrong pair": ("in_place && i == 0 && j == n - 1", "in_place && i == 0 && j == 1", "arrays_overlap"),
    "the last array is not looked at": ("for (int j = i + 1; j < n; ++j)\n      if (spans_meet",
                                        "for (int j = i + 1; j < n - 1; ++j)\n      if (spans_meet", "outputs_overlap"),
}


def compile_against(include_dir, exe):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    return subprocess.Popen([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                             "-fno-sanitize-recover=undefined", "-I", include_dir, SOURCE, "-o", exe])


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    """{None: the program built against the header, name: against the header with that mutation}, compiled side by side."""
    tmp = tmp_path_factory.mktemp("host_args")
    text = open(os.path.join(CSRC, "host_args.h")).read()
    exes, jobs = {}, []
    for k, name in enumerate([None] + sorted(MUTATIONS)):
        inc = CSRC
        if name is not None:
            old, new, _ = MUTATIONS[name]
            assert text.count(old) == 1, "the mutation %r names one place of the header" % name
            inc = str(tmp / ("mutant%d" % k))
            os.mkdir(inc)
            with open(os.path.join(inc, "host_args.h"), "w") as f:
                f.write(text.replace(old, new))
        exes[name] = str(tmp / ("host_args_host%d" % k))
        jobs.append(compile_against(inc, exes[name]))
    assert all(j.wait() == 0 for j in jobs)
    return exes


def test_every_rule_holds_its_definition(hosts):
    out = subprocess.run([hosts[None]], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    n = dict(line.split() for line in out.stdout.splitlines()[:-1])
    assert out.stdout.splitlines()[-1] == "every rule holds its definition"
    # 7 starts x 7 lengths and NULL; every pair; every list of 0 .. 4; of 0 .. 3 non-empty; 0 .. 3 outputs x 0 .. 3 inputs
    assert int(n["spans"]) == 50 and int(n["pairs"]) == 50 ** 2
    assert int(n["lists"]) == sum(50 ** k for k in range(5))
    assert int(n["sorted_lists"]) == sum(42 ** k for k in range(4))
    assert int(n["alias_lists"]) == sum(4 ** k for k in range(4)) ** 2


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_the_sweep_sees_a_changed_rule(hosts, name):
    out = subprocess.run([hosts[name]], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1, out.stdout + out.stderr
    assert out.stdout.splitlines()[-1].startswith(MUTATIONS[name][2] + " differs"), out.stdout

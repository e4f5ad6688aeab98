"""tools/sanitize/query_sanitize.cpp stays alive: built with the line its header carries (csrc/rtamd_query.hip against aborting stubs
of everything it asks of rtamd_api.hip, under the host's address and undefined-behaviour sanitizers) and run, stand-alone -- no GPU, no
Python in the process, nothing preloaded.  A launch function that rtamd_query.hip comes to need and the program has no stub for fails
the link here, and so does a refusal that moved.  Skipped where there is no hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "sanitize", "query_sanitize.cpp")


def test_the_sanitizer_program_builds_and_runs_clean(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if not hipcc:
        pytest.skip("no hipcc to build tools/sanitize/query_sanitize.cpp with")
    header = open(SOURCE).read().split("#include")[0]
    found = re.search(r"//\s+(hipcc .*?)-o \S+ && \S+\n", header, re.S)
    assert found, "the header comment of query_sanitize.cpp no longer carries its build line (hipcc ... -o PROGRAM && PROGRAM)"
    line = " ".join(part.strip(" /\\") for part in found.group(1).splitlines()).strip()
    assert "-fsanitize=address,undefined" in line and line.endswith("rtamd_query.hip"), line
    exe = tmp_path / "query_asan"
    build = subprocess.run([hipcc] + line.split()[1:] + ["-o", str(exe)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.splitlines()[-1]
    assert re.fullmatch(r"query_sanitize: \d+ refusals, all as expected", last), last
    assert int(last.split()[1]) >= 200 and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr

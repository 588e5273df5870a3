"""The layout of the native build (glim_amd/csrc): every .hip file is a translation unit of its own, every header stands alone, the Makefile
finds the sources itself and takes each unit's header dependencies from the compiler.  No GPU is needed."""
import glob
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glim_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
UNITS = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(CSRC, "*.hip")))
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.hpp")))


def make_n(*args):
    """What `make -n <args>` would run in csrc: (the units it would compile, the objects it would link or None)."""
    out = subprocess.run(["make", "-C", CSRC, "-n", *args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    compiled, linked = [], None
    for line in out.stdout.splitlines():
        m = re.search(r" -c (\S+)\.hip -o (\S+)\.o$", line)
        if m:
            assert m.group(1) == m.group(2), line
            compiled.append(m.group(1))
        elif " -shared " in line:
            assert linked is None, "two link lines"
            linked = sorted(w[:-2] for w in line.split() if w.endswith(".o"))
    assert len(compiled) == len(set(compiled)), compiled
    return sorted(compiled), linked


@pytest.fixture(scope="module")
def built():
    """The library and the dependency files beside its objects are up to date (nothing happens when they already are)."""
    from glim_amd import _lib

    _lib.build()


def test_no_source_file_includes_another_source_file():
    assert len(UNITS) >= 22
    for u in UNITS:
        text = open(os.path.join(CSRC, u + ".hip")).read()
        assert not re.search(r'^\s*#\s*include\s*[<"][^>"]*\.hip[>"]', text, re.M), u + ".hip includes a .hip file"
    assert not os.path.exists(os.path.join(CSRC, "ivox.hpp"))


def test_every_header_compiles_as_the_only_include():
    assert len(HEADERS) >= 18
    with tempfile.TemporaryDirectory() as tmp:

        def check(header):
            src = os.path.join(tmp, os.path.basename(header)[:-4] + "_alone.hip")
            with open(src, "w") as f:
                f.write(f'#include "{header}"\n')
            return header, subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", src], capture_output=True, text=True, timeout=600)

        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            for header, res in pool.map(check, HEADERS):
                assert res.returncode == 0, os.path.basename(header) + " does not stand alone:\n" + res.stderr[-2000:]


def test_make_compiles_and_links_exactly_the_source_files():
    compiled, linked = make_n("-B")
    assert compiled == UNITS
    assert linked == UNITS


def test_nothing_is_rebuilt_when_nothing_changed(built):
    assert make_n() == ([], None)


def test_an_object_older_than_the_makefile_is_rebuilt(built):
    """An object left by an earlier Makefile has no dependency file beside it: it is compiled again rather than trusted."""
    compiled, linked = make_n("-W", "Makefile")
    assert compiled == UNITS
    assert linked == UNITS


def test_a_touched_header_rebuilds_the_units_that_include_it_and_no_other(built):
    compiled, linked = make_n("-W", "lm_step.hpp")
    assert compiled == ["bundle_align", "ct_align", "gicp_align", "vgicp_align"]
    assert linked == UNITS
    compiled, _ = make_n("-W", "gicp_factor.hpp")
    assert compiled == ["ct_align", "gicp", "gicp_align", "ivox"]
    # one unit per family of loops: a family's rule rebuilds its own unit.  (keyframe_lm_step.hpp includes bundle_lm_step.hpp for the prior's
    # term, so the bundle's rule reaches vgicp_align too; no rule reaches gicp_align or ct_align but their own)
    compiled, _ = make_n("-W", "bundle_lm_step.hpp")
    assert compiled == ["bundle_align", "vgicp_align"]
    compiled, _ = make_n("-W", "keyframe_lm_step.hpp")
    assert compiled == ["vgicp_align"]
    compiled, _ = make_n("-W", "ct_lm_step.hpp")
    assert compiled == ["ct_align"]
    compiled, _ = make_n("-W", "graph_solve.hpp")
    assert compiled == ["bundle_align", "graph_solve"]
    compiled, _ = make_n("-W", "vgicp_batch.hpp")
    assert compiled == ["bundle_align", "vgicp", "vgicp_align"]
    # the global registration: gnc.hip stands on ransac.hip's table, both on fpfh.hip's matcher
    compiled, _ = make_n("-W", "ransac_table.hpp")
    assert compiled == ["gnc", "ransac"]
    compiled, _ = make_n("-W", "fpfh.hpp")
    assert compiled == ["fpfh", "gnc", "ransac"]

"""The device ingest path's switches (include/drephip.h: drephip_set_ingest_path,
DREPHIP_INGEST) and its text tile size.  Creating a context needs a HIP device,
so the context parts are marked gpu; the rest runs without one."""
import os
import subprocess
import sys

import pytest

from drep_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_text_tile_bytes_is_a_power_of_two():
    T = _lib.text_tile_bytes()
    assert T >= 4096 and T & (T - 1) == 0
    # a tile of text never yields more bases than one sketch tile holds
    assert T <= _lib.tile_bases()


def test_text_layout_aligns_file_starts():
    starts, off = _lib.text_layout([5, 0, 16, 33, 1])
    assert list(starts) == [0, 16, 16, 32, 80] and list(off) == [0, 5, 16, 32, 65, 81]
    assert all(int(s) % 16 == 0 for s in starts)


def test_ingest_kwarg_is_checked_before_any_work(tmp_path):
    import pandas as pd
    from drep_amd import d_cluster
    Bdb = pd.DataFrame({"genome": ["a.fa"], "location": [str(tmp_path / "a.fa")]})
    with pytest.raises(ValueError):
        d_cluster.sketch_genomes(Bdb, str(tmp_path), ingest="x")


def test_ingest_kwarg_is_checked_on_a_dry_run(tmp_path):
    import pandas as pd
    from drep_amd import d_cluster
    Bdb = pd.DataFrame({"genome": ["a.fa"], "location": [str(tmp_path / "a.fa")]})
    with pytest.raises(ValueError):
        d_cluster.all_vs_all_MASH(Bdb, str(tmp_path), dry=True, ingest="gpu")


def _host_program(tmp_path, source, name, sanitize, libs=()):
    """`source` built as a stand-alone host program with -fsanitize=`sanitize`."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / name
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                    "-fsanitize=" + sanitize, "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "drep_amd", "csrc"), str(source), "-o", str(exe), *libs],
                   check=True, capture_output=True, cwd=tmp_path)
    return exe


def test_byte_machine_and_tile_lists_on_the_host(tmp_path):
    """tools/fasta_machine_check.cpp: the kernels' lane / tile decomposition, the
    pack call's tile and chunk lists and the kernels' search in them, replayed
    on the CPU through the inline functions the kernels call
    (csrc/fasta_machine.h), as a stand-alone host program built with the
    address and undefined-behaviour sanitizers."""
    exe = _host_program(tmp_path, os.path.join(ROOT, "tools", "fasta_machine_check.cpp"), "fasta_machine_check",
                        "address,undefined")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert ", 0 disagree" in out.stdout and not out.stderr.strip(), out.stdout + out.stderr


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_ingest_pipeline_machinery_on_the_host(tmp_path, sanitize):
    """tools/ingest_pipeline_check.cpp: the producer / consumer driver of
    drephip_sketch_files under fake stages (order, slot ownership, an error on
    either side with the other parked or mid-batch), its batch plan and its
    worker pool (csrc/ingest_pipeline.h), as a stand-alone host program: once
    with the address and undefined-behaviour sanitizers, once with the thread
    sanitizer."""
    if sanitize == "thread":
        # skipped only where the thread sanitizer's runtime itself cannot start
        trivial = tmp_path / "trivial.cpp"
        trivial.write_text("#include <thread>\nint main() { int x = 0; std::thread t([&] { x = 1; }); t.join();\n"
                           "  return x - 1; }\n")
        probe = subprocess.run([str(_host_program(tmp_path, trivial, "trivial", sanitize))], capture_output=True,
                               text=True, timeout=60)
        if probe.returncode != 0:
            pytest.skip("a three-line program built with -fsanitize=thread cannot start here (the runtime refuses "
                        "the address layout): " + probe.stderr.strip()[:200])
    exe = _host_program(tmp_path, os.path.join(ROOT, "tools", "ingest_pipeline_check.cpp"), "ingest_pipeline_check",
                        sanitize, libs=["-lz"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert ", 0 disagree" in out.stdout and not out.stderr.strip(), out.stdout + out.stderr


def test_api_argument_checks_on_the_host(tmp_path):
    """tools/api_checks_check.cpp: the C API's pure argument checks
    (csrc/api_checks.h) -- the row check at every nhash with a violation at the
    first and last position of a row and of the matrix, the triangle's row
    range against a brute-force pair count, the permutation and distance-table
    checks -- as a stand-alone host program built with the address and
    undefined-behaviour sanitizers."""
    exe = _host_program(tmp_path, os.path.join(ROOT, "tools", "api_checks_check.cpp"), "api_checks_check",
                        "address,undefined")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " checks, 0 disagree" in out.stdout and not out.stderr.strip(), out.stdout + out.stderr


def test_set_ingest_path_needs_a_context():
    L = _lib.lib()
    assert L.drephip_set_ingest_path(None, 0) == -1 and L.drephip_last_error()
    assert L.drephip_last_ingest_paths(None, None, None, None) == -1


@pytest.mark.gpu
def test_new_context_is_on_the_host_path(monkeypatch):
    monkeypatch.delenv("DREPHIP_INGEST", raising=False)
    L = _lib.lib()
    with _lib.Context(0, 21, 1000, 42) as ctx:
        assert ctx.ingest_path == "host"
        assert ctx.ingest_paths() == {"path": "host", "device_files": 0, "host_files": 0, "text_bytes": 0}
        assert L.drephip_set_ingest_path(ctx.handle, 7) == -1 and L.drephip_last_error()
        assert L.drephip_set_ingest_path(ctx.handle, -1) == -1
        assert ctx.ingest_path == "host"
        ctx.set_ingest_path("device")
        assert ctx.ingest_path == "device"
        ctx.sketch_files([])                                           # a zero-file call keeps the path
        assert ctx.ingest_paths()["path"] == "device"
        ctx.set_ingest_path("host")
        assert ctx.ingest_path == "host"


@pytest.mark.gpu
@pytest.mark.parametrize("value,want", [("device", "device"), ("host", "host"), ("nonsense", "host")])
def test_environment_names_a_new_contexts_path(value, want):
    code = ("from drep_amd import _lib\n"
            "with _lib.Context(0, 21, 1000, 42) as c:\n"
            "    print(c.ingest_path)\n")
    env = dict(os.environ, DREPHIP_INGEST=value, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == want

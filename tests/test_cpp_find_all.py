"""kh::ShardedTable::find_all (include/cs267_hw3_amd/dist_hash_map.hpp) on the GPU: the batched,
collective find of the C++ host. tests/cpp/test_find_all.cpp is compiled here (the flags of
tests/cpp/Makefile) and run at P = 1, 2, 3 thread ranks with a peer group, and once without one;
inside the program every rank's records and found flags are compared with the records parsed from
the input text, for present and absent keys."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
pytestmark = pytest.mark.gpu

_built = {}


def _exe(k, tmp_path_factory):
    if k not in _built:
        out = str(tmp_path_factory.mktemp(f"find_all_{k}") / f"test_find_all_{k}")
        libdir = os.path.join(ROOT, "cs267_hw3_amd")
        cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", f"-DKMER_LEN={k}",
               "-D__HIP_PLATFORM_AMD__", f"-I{ROOT}/include", f"-I{ROCM}/include",
               os.path.join(ROOT, "tests", "cpp", "test_find_all.cpp"), "-o", out,
               f"-L{libdir}", "-lkmerhash_amd", f"-Wl,-rpath,{libdir}", f"-L{ROCM}/lib", "-lamdhip64", "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        _built[k] = out
    return _built[k]


def _run(exe, name, P, peers):
    r = subprocess.run([exe, os.path.join(GOLDEN, f"{name}.txt"), str(P), str(peers)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "find_all ok" in r.stdout


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("name,k", [("tiny19", 19), ("small51", 51)])
def test_find_all_peer_group(tmp_path_factory, name, k, P):
    _run(_exe(k, tmp_path_factory), name, P, 1)


@pytest.mark.parametrize("name,k,P", [("small51", 51, 3), ("tiny19", 19, 2)])
def test_find_all_without_peer_group(tmp_path_factory, name, k, P):
    """One process per GPU has no peer group: the same exchanges, nothing read from a peer's table."""
    _run(_exe(k, tmp_path_factory), name, P, 0)

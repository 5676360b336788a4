"""The container layer of the LIBRARY under the host sanitizers, as a stand-alone program (tests/host_san/frames_main.cpp): the
library's .cpp files compiled with the address and undefined-behaviour sanitizers on their host side, linked with the plain device
objects of the normal build (swcompression_amd/build/*.hip.o; compiled here where a tree has none).  The recipe lives here, not
in swcompression_amd/build.py: the product is never built this way.  Run as a child process, never loaded into python; nothing goes
into LD_PRELOAD.  TEST INFRASTRUCTURE ONLY."""
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

from swcompression_amd import build as B

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_MAIN = os.path.join(_HERE, "host_san", "frames_main.cpp")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
KIND = {"gzip": 1, "zlib": 2, "lz4": 4, "bzip2": 5, "xz": 6}   # as swc_unarchive_many counts them


def case_file(cases):
    """The bytes frames_main reads (its header comment has the layout)."""
    out = bytearray(struct.pack("<I", len(cases)))
    for c in cases:
        d = b"" if c.dictionary is None else bytes(c.dictionary)
        name = ("%s/%s" % (c.kind, c.name)).encode()
        out += struct.pack("<IIiIqI", KIND[c.kind], 1 if c.stage == "header" else 0, c.status, 0 if c.dictionary is None else 1,
                           -1 if c.dict_id is None else c.dict_id, len(d)) + d
        out += struct.pack("<I", len(name)) + name + struct.pack("<I", len(c.data)) + c.data
    return bytes(out)


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_program(tmp_path):
    """-> the path of the program."""
    common = [_hipcc(), "--offload-arch=" + B.ARCH, "-O1", "-g", "-std=c++17", "-fPIC", "-x", "hip"]
    jobs, objs = [], []
    for src in B.sources() + [_MAIN]:
        base = os.path.basename(src)
        if src.endswith(".hip"):
            obj = os.path.join(B.HERE, "build", base + ".o")       # the device code as the product has it: no sanitizer in kernels
            if not (os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(p) for p in B._deps())):
                obj = str(tmp_path / (base + ".o"))
                jobs.append([_hipcc(), "--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", src, "-o", obj])
        else:
            obj = str(tmp_path / (base + ".san.o"))
            jobs.append(common + SANITIZE + ["-I", os.path.join(_ROOT, "include"), "-c", src, "-o", obj])
        objs.append(obj)
    with ThreadPoolExecutor(min(len(jobs), 16)) as ex:
        for p in ex.map(lambda cmd: subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), jobs):
            assert p.returncode == 0, p.stdout[-4000:]
    exe = str(tmp_path / "frames_main")
    # (the link, too, asks for the sanitizers' runtime on the host side only: the device code stays as the product has it)
    p = subprocess.run([_hipcc(), "--offload-arch=" + B.ARCH] + SANITIZE[:2] + ["-o", exe] + objs,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    return exe


def run_program(exe, tmp_path, cases, timeout=600):
    """The program once on `cases`: asserts that it ends with status 0 and returns what it printed."""
    path = str(tmp_path / "frames_cases.bin")
    with open(path, "wb") as f:
        f.write(case_file(cases))
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, errors="replace", timeout=timeout)
    assert p.returncode == 0, p.stdout[-6000:]
    return p.stdout

"""How the suite builds and runs its stand-alone programs: libjpeg 9 itself (tests/libjpeg9_*.c) and the host builds of
csrc/*.h (tests/*_host.cpp).  One compiler lookup, one sanitizer flag list, one build with a per-process cache, one way to
run a program and to fail a test on what it did.  The programs are processes of their own: nothing built here is ever
loaded into Python.  The byte formats of their case files are in tests/wire.py."""
import atexit
import hashlib
import itertools
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
CSRC = HERE.parent / "jpeg-quantsmooth_amd" / "csrc"
JPEGINC = Path("/opt/conda/include")
JPEGLIB = Path("/opt/conda/lib/libjpeg.so.9")
# sanitize=True: every bad read or write, and every undefined operation, ends the program with a report on stderr
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

_built = {}                        # (digest of the source, the command line) -> executable
_root = None                       # where they are, removed at exit
_serial = itertools.count(1)       # of the case files of this process: no two tools share a name


def compiler(cxx: bool) -> str:
    if cxx:
        return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"
    return os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc") or "gcc"


def build(source, flags=(), defines=(), sanitize=False, libjpeg=False) -> Path:
    """tests/<source> as a program -> its path.  C or C++17 by the suffix, -O2 -Wall unless `flags` (which come later on
    the line) or `sanitize` (SANITIZE) say otherwise; csrc/ is on the include path, with `libjpeg` libjpeg 9 as well, and
    the program links it.  Each distinct (source text, command line) is compiled once per process; a compiler error
    fails the test with the compiler's words."""
    global _root
    src = HERE / source
    cxx = src.suffix == ".cpp"
    cmd = [compiler(cxx), *(["-std=c++17"] if cxx else []), "-Wall", *(SANITIZE if sanitize else ["-O2"]), *flags,
           *(f"-D{d}" for d in defines), f"-I{CSRC}", *([f"-I{JPEGINC}"] if libjpeg else []), str(src),
           *([str(JPEGLIB), f"-Wl,-rpath,{JPEGLIB.parent}"] if libjpeg else [])]
    key = (hashlib.sha256(src.read_bytes()).hexdigest(), tuple(cmd))
    if key not in _built:
        if _root is None:
            _root = Path(tempfile.mkdtemp(prefix="qs_host_tools_"))
            atexit.register(shutil.rmtree, _root, ignore_errors=True)
        exe = _root / str(len(_built)) / "_".join([src.stem, *(["san"] if sanitize else []), *defines])
        exe.parent.mkdir()
        r = subprocess.run([*cmd, "-o", str(exe)], capture_output=True, text=True)
        if r.returncode or not exe.exists():
            pytest.fail(f"tests/{source} did not build ({exe.name}):\n{r.stderr}")
        _built[key] = exe
    return _built[key]


def run(exe, *args, ok=(0,), silent=False):
    """the program on the arguments -> the completed process.  An exit status outside `ok` (None: any is the caller's to
    read) fails the test, and with `silent` so does anything on stderr: that is how a sanitizer report fails a test."""
    r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
    if (ok is not None and r.returncode not in ok) or (silent and r.stderr):
        pytest.fail(f"{Path(exe).name} {' '.join(map(str, args[:2]))} failed (exit {r.returncode}):\n"
                    f"{r.stdout[-1000:]}{r.stderr[-4000:]}")
    return r


class Tool:
    """a built program and the directory its case files go to.  SILENT: a run that writes to stderr fails."""
    SILENT = False

    def __init__(self, exe, workdir):
        self.exe, self.dir = Path(exe), Path(workdir)

    def tmp(self, ext) -> Path:
        return self.dir / f"{self.exe.name}_{os.getpid()}_{next(_serial)}{ext}"

    def _run(self, *args, ok=(0,)):
        return run(self.exe, *args, ok=ok, silent=self.SILENT)

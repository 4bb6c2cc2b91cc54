"""Build the in-tree native extensions (no JIT cache — the .so files live
in the package directory so they travel with the source tree).

- ``_amdhal``: plain C++ (g++/amdclang++), links libamd_smi.
- ``_hiphealth``: HIP, compiled for gfx950 only (hipcc cross-compiles
  without a GPU present).
- ``_claimio``: plain C++, no external link; the prepare path's JSON
  encoding, checksum and atomic file writes.
"""

from __future__ import annotations

import os
import subprocess
import sys
import sysconfig

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CPP_DIR = os.path.join(PKG_DIR, "cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
GPU_ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def _ext_suffix() -> str:
    return sysconfig.get_config_var("EXT_SUFFIX") or ".so"


def _pybind_includes() -> list:
    import pybind11

    return [f"-I{pybind11.get_include()}", f"-I{sysconfig.get_paths()['include']}"]


def _needs_build(src: str, out: str) -> bool:
    return not os.path.exists(out) or os.path.getmtime(src) > os.path.getmtime(out)


def _run(cmd: list) -> None:
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def build_amdhal(force: bool = False) -> str:
    src = os.path.join(CPP_DIR, "amdhal.cpp")
    out = os.path.join(PKG_DIR, f"_amdhal{_ext_suffix()}")
    if force or _needs_build(src, out):
        _run(
            ["g++", "-shared", "-fPIC", "-O2", "-std=c++17"]
            + _pybind_includes()
            + [
                f"-I{ROCM}/include",
                src,
                f"-L{ROCM}/lib",
                "-lamd_smi",
                f"-Wl,-rpath,{ROCM}/lib",
                "-o",
                out,
            ]
        )
    return out


def build_amdhal_asan(force: bool = False) -> str:
    """AddressSanitizer flavor of the amdsmi binding (the
    cgo-shim ASan build the reference's pure-Go stack never needed).
    Run it with:
        LD_PRELOAD=$(gcc -print-file-name=libasan.so) \
        ASAN_OPTIONS=detect_leaks=0 python -c 'import ... _amdhal_asan'
    (leak detection off: the Python interpreter itself 'leaks' at exit).
    """
    src = os.path.join(CPP_DIR, "amdhal.cpp")
    out = os.path.join(PKG_DIR, f"_amdhal_asan{_ext_suffix()}")
    if force or _needs_build(src, out):
        _run(
            [
                "g++",
                "-shared",
                "-fPIC",
                "-g",
                "-O1",
                "-std=c++17",
                "-fsanitize=address",
                "-fno-omit-frame-pointer",
                "-DPYBIND11_MODULE_NAME=_amdhal_asan",
            ]
            + _pybind_includes()
            + [
                f"-I{ROCM}/include",
                src,
                f"-L{ROCM}/lib",
                "-lamd_smi",
                f"-Wl,-rpath,{ROCM}/lib",
                "-o",
                out,
            ]
        )
    return out


def build_hiphealth(force: bool = False) -> str:
    """HIP kernels; rebuilt when the source or a header it includes (the
    self-test's, the CU footprint's, the per-CU self-test's, the load
    self-test's, the MX load self-test's, the HBM march's) changes."""
    src = os.path.join(CPP_DIR, "hiphealth.hip")
    hdrs = [
        os.path.join(CPP_DIR, "selftest_kernels.hpp"),
        os.path.join(CPP_DIR, "footprint_kernels.hpp"),
        os.path.join(CPP_DIR, "cutest_kernels.hpp"),
        os.path.join(CPP_DIR, "loadtest_kernels.hpp"),
        os.path.join(CPP_DIR, "loadtest_core.hpp"),
        os.path.join(CPP_DIR, "mxtest_kernels.hpp"),
        os.path.join(CPP_DIR, "mxtest_core.hpp"),
        os.path.join(CPP_DIR, "hbmtest_kernels.hpp"),
        os.path.join(CPP_DIR, "hbmtest_core.hpp"),
    ]
    out = os.path.join(PKG_DIR, f"_hiphealth{_ext_suffix()}")
    if force or _needs_build(src, out) or any(_needs_build(h, out) for h in hdrs):
        hipcc = os.path.join(ROCM, "bin", "hipcc")
        if not os.path.exists(hipcc):
            hipcc = "hipcc"
        _run(
            [
                hipcc,
                f"--offload-arch={GPU_ARCH}",
                "-shared",
                "-fPIC",
                "-O3",
                "-std=c++17",
            ]
            + _pybind_includes()
            + [src, "-o", out]
        )
    return out


def build_claimio(force: bool = False) -> str:
    """Claim persistence (JSON encode + checksum + atomic write); plain
    C++, no ROCm link. Rebuilt when either the binding or its Python-free
    core header changes."""
    src = os.path.join(CPP_DIR, "claimio.cpp")
    hdr = os.path.join(CPP_DIR, "claimio_core.hpp")
    out = os.path.join(PKG_DIR, f"_claimio{_ext_suffix()}")
    if force or _needs_build(src, out) or _needs_build(hdr, out):
        _run(
            ["g++", "-shared", "-fPIC", "-O2", "-std=c++17"]
            + _pybind_includes()
            + [src, "-o", out]
        )
    return out


def _gcc_file(name: str) -> str:
    """Absolute path of a gcc support file, "" when it is not installed."""
    try:
        out = subprocess.run(
            ["gcc", f"-print-file-name={name}"],
            capture_output=True,
            text=True,
            check=True,
        ).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return ""
    return out if os.path.isabs(out) else ""


def sanitizer_link_flags():
    """Link flags for an ASan+UBSan executable, or None when gcc has no
    sanitizer runtime installed. The static runtimes are preferred: the
    program then carries its sanitizer with it and does not depend on the
    order in which shared libraries are loaded into the process."""
    if _gcc_file("libasan.a") and _gcc_file("libubsan.a"):
        return ["-static-libasan", "-static-libubsan"]
    if _gcc_file("libasan.so") and _gcc_file("libubsan.so"):
        return []
    return None


def build_claimio_selftest(out: str, sanitize: bool = True) -> str:
    """Stand-alone driver of claimio_core.hpp (its own ``main``, no
    Python), by default under AddressSanitizer + UBSan. CPU only; run the
    binary directly."""
    src = os.path.join(CPP_DIR, "claimio_selftest.cpp")
    flags = ["-g", "-O1", "-std=c++17"]
    if sanitize:
        link = sanitizer_link_flags()
        if link is None:
            raise RuntimeError("gcc has no ASan/UBSan runtime installed")
        flags += [
            "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined",
            "-fno-omit-frame-pointer",
        ] + link
    _run(["g++"] + flags + [src, "-o", out])
    return out


def build_loadtest_core_selftest(out: str, sanitize: bool = True) -> str:
    """Stand-alone driver of loadtest_core.hpp (the load self-test's operand
    generator, K bound and checksum; its own ``main``, no Python, no HIP),
    by default under AddressSanitizer + UBSan. CPU only; run the binary
    directly."""
    src = os.path.join(CPP_DIR, "loadtest_core_selftest.cpp")
    flags = ["-g", "-O1", "-std=c++17"]
    if sanitize:
        link = sanitizer_link_flags()
        if link is None:
            raise RuntimeError("gcc has no ASan/UBSan runtime installed")
        flags += [
            "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined",
            "-fno-omit-frame-pointer",
        ] + link
    _run(["g++"] + flags + [src, "-o", out])
    return out


def build_mxtest_core_selftest(out: str, sanitize: bool = True) -> str:
    """Stand-alone driver of mxtest_core.hpp (the MX load self-test's element
    and scale formats, operand generator, K bounds and checksum; its own
    ``main``, no Python, no HIP), by default under AddressSanitizer + UBSan.
    CPU only; run the binary directly."""
    src = os.path.join(CPP_DIR, "mxtest_core_selftest.cpp")
    flags = ["-g", "-O1", "-std=c++17"]
    if sanitize:
        link = sanitizer_link_flags()
        if link is None:
            raise RuntimeError("gcc has no ASan/UBSan runtime installed")
        flags += [
            "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined",
            "-fno-omit-frame-pointer",
        ] + link
    _run(["g++"] + flags + [src, "-o", out])
    return out


def build_hbmtest_core_selftest(out: str, sanitize: bool = True) -> str:
    """Stand-alone driver of hbmtest_core.hpp (the HBM march's chunk plan,
    round schedule, expected word and report aggregation; its own ``main``,
    no Python, no HIP), by default under AddressSanitizer + UBSan. CPU only;
    run the binary directly."""
    src = os.path.join(CPP_DIR, "hbmtest_core_selftest.cpp")
    flags = ["-g", "-O1", "-std=c++17"]
    if sanitize:
        link = sanitizer_link_flags()
        if link is None:
            raise RuntimeError("gcc has no ASan/UBSan runtime installed")
        flags += [
            "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined",
            "-fno-omit-frame-pointer",
        ] + link
    _run(["g++"] + flags + [src, "-o", out])
    return out


def build(force: bool = False) -> None:
    build_amdhal(force)
    build_hiphealth(force)
    build_claimio(force)


if __name__ == "__main__":
    build(force="--force" in sys.argv)

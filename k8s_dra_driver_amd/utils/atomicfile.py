"""Atomic small-file persistence helpers (checkpoints, CDI specs).

Hot-path notes (the prepare path writes two of these per claim): the
original implementation paid ``tempfile.mkstemp`` (random-name loop +
O_EXCL probing, ~3% of lifecycle CPU in the sampling profile) and a
``makedirs`` per write. Temp names here are unique by construction
(pid + per-process counter — collisions impossible within a process,
and cross-process names differ by pid), and directory existence is
memoized (directories are created once per process lifetime; an
externally deleted parent resurfaces as ENOENT and retries once).

The syscall sequence itself (open/write/fsync/close/rename) and the
compact JSON encoding run in the ``_claimio`` extension when it is built:
one GIL release per file instead of one per syscall. The Python
implementation below stays as the fallback and as the reference the
native path is tested against byte for byte; using it is never silent.
"""

from __future__ import annotations

import itertools
import json
import logging
import os
import threading
from typing import Any

log = logging.getLogger(__name__)

try:
    from .. import _claimio as _native_mod
except ImportError as _e:  # not built: build_native.build_claimio()
    _native_mod = None
    _native_import_error = str(_e)
else:
    _native_import_error = ""

_native_on = _native_mod is not None
_fallback_warned = False

_counter = itertools.count()
_known_dirs = set()
_dirs_lock = threading.Lock()


def set_native(on: bool) -> bool:
    """Switch between the ``_claimio`` path and the Python path (tests
    force either one). Returns the previous setting; asking for the native
    path when the extension is not built raises."""
    global _native_on
    if on and _native_mod is None:
        raise RuntimeError(
            f"_claimio extension not available: {_native_import_error}"
        )
    prev, _native_on = _native_on, bool(on)
    return prev


def native():
    """The ``_claimio`` module, or None when the Python path is in force
    (logged once per process: this project does not fall back silently)."""
    global _fallback_warned
    if _native_on:
        return _native_mod
    if not _fallback_warned:
        _fallback_warned = True
        log.warning(
            "claim persistence is running on the pure-Python path (%s); "
            "expect a slower prepare",
            _native_import_error or "native path switched off",
        )
    return None


def _ensure_dir(d: str) -> None:
    if d in _known_dirs:
        return
    os.makedirs(d, exist_ok=True)
    with _dirs_lock:
        _known_dirs.add(d)


def _tmp_name(path: str) -> str:
    d = os.path.dirname(path)
    return os.path.join(d, f".tmp-{os.getpid()}-{next(_counter)}")


def atomic_write_bytes(path: str, data: bytes, *, durable: bool = True) -> None:
    """tmp + fsync + rename so a crash can never leave a torn file.

    ``durable=False`` skips the fsync (rename atomicity is kept: readers
    never see a torn file, but the content may be lost on power failure).
    Only correct for files that are REGENERABLE from durable state —
    e.g. per-claim CDI specs, which DeviceState rebuilds from the
    checkpoint on the prepare cache-hit path. fsync is ~10% of the
    prepare hot path on the MI355X pool boxes (sampling profile,
    profiles/round2_hardware_notes.md)."""
    d = os.path.dirname(path)
    _ensure_dir(d)
    tmp = _tmp_name(path)
    nat = native()
    if nat is not None:
        try:
            nat.write_replace(tmp, path, data, durable)
        except FileNotFoundError as e:
            if e.filename != tmp:
                raise
            # parent deleted externally since we memoized it: recreate
            with _dirs_lock:
                _known_dirs.discard(d)
            _ensure_dir(d)
            nat.write_replace(tmp, path, data, durable)
        return
    try:
        fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_EXCL, 0o644)
    except FileNotFoundError:
        # parent deleted externally since we memoized it: recreate
        with _dirs_lock:
            _known_dirs.discard(d)
        _ensure_dir(d)
        fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_EXCL, 0o644)
    try:
        os.write(fd, data)
        if durable:
            os.fsync(fd)
        os.close(fd)
        fd = -1
        os.replace(tmp, path)
    except BaseException:
        if fd >= 0:
            os.close(fd)
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def atomic_write_text(path: str, data: str, *, durable: bool = True) -> None:
    """``atomic_write_bytes`` of the UTF-8 encoding of ``data``."""
    atomic_write_bytes(path, data.encode(), durable=durable)


def encode_json(obj: Any, indent=None) -> bytes:
    """Canonical (sorted-key) JSON bytes: compact when ``indent`` is None,
    else indented as ``json.dumps(indent=indent)``. The native encoder
    refuses (TypeError) whatever it would not render exactly as
    ``json.dumps`` does, and that input takes the stock encoder."""
    nat = native()
    if nat is not None:
        try:
            return nat.encode(obj, indent)
        except TypeError:
            pass
    if indent is None:
        return json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()
    return json.dumps(obj, indent=indent, sort_keys=True).encode()


def atomic_write_json(path: str, obj: Any) -> None:
    atomic_write_bytes(path, encode_json(obj))


def read_json(path: str) -> Any:
    with open(path) as f:
        return json.load(f)

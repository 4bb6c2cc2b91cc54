"""The _claimio extension against the Python code it replaces.

Every byte the native path produces — encoder output, checkpoint files,
claim CDI specs — must equal what json.dumps / the Python atomic writer
produce for the same input; ``atomicfile.set_native`` forces either path.
All CPU; no GPU needed.
"""

import dataclasses
import errno
import json
import os
import random
import re
import shutil
import subprocess
import threading
import zlib

import pytest

from k8s_dra_driver_amd.cdi.handler import CDIHandler
from k8s_dra_driver_amd.cdi.spec import ContainerEdits, Mount
from k8s_dra_driver_amd.state.checkpoint import (
    CheckpointCorrupt,
    CheckpointStore,
    PreparedClaim,
    PreparedDevice,
    _checksum,
)
from k8s_dra_driver_amd.utils import atomicfile


@pytest.fixture(scope="module")
def claimio():
    from k8s_dra_driver_amd import _claimio  # build() must have produced it

    return _claimio


@pytest.fixture
def native_switch():
    """set_native, restored afterwards."""
    prev = atomicfile.set_native(True)
    yield atomicfile.set_native
    atomicfile.set_native(prev)


def py_compact(obj) -> bytes:
    return json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()


def py_indent(obj, indent=2) -> bytes:
    return json.dumps(obj, indent=indent, sort_keys=True).encode()


def _device(i: int, name: str = "") -> PreparedDevice:
    return PreparedDevice(
        request_names=["gpu", f"req-{i}"] if i % 2 else [],
        pool_name="nœud-1" if i == 0 else "node-1",
        device_name=name or f"gpu-{i}",
        cdi_device_ids=[
            f"k8s.gpu.amd.com/device=gpu-{i}",
            f"k8s.gpu.amd.com/claim=uid-gpu-{i}",
        ],
        parent_gpu_index=i if i != 3 else -1,
        kind="partition" if i % 3 == 2 else "gpu",
        device_uuid=f"GPU-{i:04x}-é",
        admin=(i == 5),
    )


def _claim(n_devices: int) -> PreparedClaim:
    return PreparedClaim(
        claim_uid=f"uid-{n_devices}",
        namespace="défault",
        name="claim-名前-\U0001f600",
        devices=[_device(i) for i in range(n_devices)],
        sharing_strategy="SharedCompute" if n_devices else "",
        timeslice_gpus=list(range(n_devices)),
        shared_session_id="sess-1" if n_devices else "",
        repartitioned={"0": ["SPX", "NPS1", "CPX", "NPS4"], "10": ["SPX", "NPS1", "DPX", "NPS2"]},
        claim_env=["AMD_DRA_CLAIM_UID=uid", 'QUOTED="a\\b"', "HSA_CU_MASK=0:0-63"],
        claim_mounts=[
            Mount(host_path="/var/run/amd-dra/shm/ü", container_path="/dev/shm/amd").to_json(),
            Mount(host_path="/opt/rocm", container_path="/opt/rocm", options=[]).to_json(),
        ],
    )


CLAIMS = [_claim(0), _claim(1), _claim(8)]

FIXED_CORPUS = [
    {},
    [],
    [[]],
    [{}],
    {"a": {}, "b": [], "c": [[], {}, [[]]], "d": {"e": {}}},
    'quote " backslash \\ both \\" end',
    "".join(chr(c) for c in range(0x00, 0x20)),
    "\x7f",
    "a\x7fb\x80c",
    "é",
    "café \u2028 \u2029 line seps",
    "\U0001f600 emoji",
    "lone \ud800 surrogate",
    "\udc00\ud800 reversed pair",
    "\uffff and \U00010000 and \U0010ffff",
    {"\uffff": 1, "\U00010000": 2},
    {"\uffff": 1, "\U00010000": 2, "a": 3, "é": 4, "": 5, "A": 6, "aa": 7},
    0,
    -1,
    2**63 - 1,
    -(2**63),
    2**63,
    -(2**63) - 1,
    2**64 + 1,
    -(10**40),
    True,
    False,
    None,
    [True, False, None, 1, 0],
    {"true": True, "one": 1},
    (1, "two", (3, ()), [4]),
    {"tuple": (1, 2), "nested": {"t": ((),)}},
    {"k": [1, {"z": "\n", "a": ["\t", {"deep": [[], [{}]]}]}]},
]


def _random_corpus(n: int):
    rng = random.Random(20240611)
    alphabet = (
        'abcXYZ019 _-./="\\\n\r\t\b\f\x00\x1f\x7f\x80éÿĀ'
        "\u2028\U000103ff\uffff\U00010000\U0001f600\U0010ffff"
    )

    def rstr():
        return "".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 12)))

    def rint():
        return rng.choice(
            [
                rng.randrange(-10, 10),
                rng.randrange(-(2**31), 2**31),
                rng.randrange(-(2**63), 2**63),
                rng.randrange(-(2**70), 2**70),
            ]
        )

    def rval(depth):
        kinds = ["none", "bool", "int", "str"]
        if depth < 4:
            kinds += ["list", "tuple", "dict", "dict", "list"]
        k = rng.choice(kinds)
        if k == "none":
            return None
        if k == "bool":
            return rng.random() < 0.5
        if k == "int":
            return rint()
        if k == "str":
            return rstr()
        if k == "list":
            return [rval(depth + 1) for _ in range(rng.randrange(0, 5))]
        if k == "tuple":
            return tuple(rval(depth + 1) for _ in range(rng.randrange(0, 4)))
        return {rstr(): rval(depth + 1) for _ in range(rng.randrange(0, 5))}

    return [rval(rng.randrange(0, 3)) for _ in range(n)]


# ---------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------


class TestEncode:
    @pytest.mark.parametrize("idx", range(len(FIXED_CORPUS)))
    def test_fixed_corpus_both_modes(self, claimio, idx):
        obj = FIXED_CORPUS[idx]
        assert claimio.encode(obj, None) == py_compact(obj)
        assert claimio.encode(obj) == py_compact(obj)
        assert claimio.encode(obj, 2) == py_indent(obj, 2)
        for indent in (0, 1, 4):
            assert claimio.encode(obj, indent) == py_indent(obj, indent)

    def test_output_is_ascii(self, claimio):
        for obj in FIXED_CORPUS:
            claimio.encode(obj, None).decode("ascii")
            claimio.encode(obj, 2).decode("ascii")

    def test_key_order_is_code_point_not_utf16(self, claimio):
        # in UTF-16 the surrogate pair of U+10000 (d800 dc00) sorts BEFORE
        # U+FFFF; by code point it sorts after
        out = claimio.encode({"\U00010000": 2, "\uffff": 1}, None)
        assert out == b'{"\\uffff":1,"\\ud800\\udc00":2}'

    def test_random_structures(self, claimio):
        corpus = _random_corpus(2000)
        assert any(isinstance(o, dict) and o for o in corpus)
        for obj in corpus:
            assert claimio.encode(obj, None) == py_compact(obj), obj
            assert claimio.encode(obj, 2) == py_indent(obj), obj

    @pytest.mark.parametrize("claim", CLAIMS, ids=["0dev", "1dev", "8dev"])
    def test_dataclass_is_encoded_as_asdict(self, claimio, claim):
        v1 = dataclasses.asdict(claim)
        assert claimio.encode(claim, None) == py_compact(v1)
        assert claimio.encode(claim, 2) == py_indent(v1)
        # nested in plain containers too, as asdict recurses
        wrapped = {"claims": [claim, (claim,)], "n": 1}
        assert claimio.encode(wrapped, None) == py_compact(
            {"claims": [v1, [v1]], "n": 1}
        )

    def test_dataclass_classvar_and_inheritance(self, claimio):
        from typing import ClassVar

        @dataclasses.dataclass
        class Base:
            z: int = 1
            shared: ClassVar[int] = 7

        @dataclasses.dataclass
        class Child(Base):
            a: str = "x"
            inner: Base = dataclasses.field(default_factory=Base)

        c = Child()
        assert claimio.encode(c, None) == py_compact(dataclasses.asdict(c))
        with pytest.raises(TypeError):
            claimio.encode(Child, None)  # the class itself is no instance

    @pytest.mark.parametrize(
        "bad",
        [
            {1: "int key"},
            {"ok": {None: 1}},
            {("a",): 1},
            {1, 2},
            frozenset(),
            object(),
            [1, object()],
            1.5,
            {"f": float("nan")},
            b"bytes",
        ],
        # repr without the address of object(): a test id must not change
        # from one run to the next
        ids=lambda bad: re.sub(r" at 0x[0-9a-f]+", "", repr(bad)),
    )
    def test_unsupported_raises_typeerror(self, claimio, bad):
        with pytest.raises(TypeError):
            claimio.encode(bad, None)
        with pytest.raises(TypeError):
            claimio.encode(bad, 2)

    def test_cycle_raises_instead_of_overflowing(self, claimio):
        a = []
        a.append(a)
        with pytest.raises(TypeError):
            claimio.encode(a, None)

    @pytest.mark.parametrize("claim", CLAIMS, ids=["0dev", "1dev", "8dev"])
    def test_encode_checkpoint(self, claimio, claim):
        v1 = claim.to_v1()
        want = py_compact({"version": 1, "checksum": _checksum(v1), "v1": v1})
        assert claimio.encode_checkpoint(claim, 1) == want
        want7 = py_compact({"version": 7, "checksum": _checksum(v1), "v1": v1})
        assert claimio.encode_checkpoint(claim, 7) == want7

    def test_encode_checkpoint_small_crc_is_not_padded(self, claimio):
        # the checksum is spliced into a fixed-width slot; short values
        # must not leave padding behind
        for obj in ({}, [], "a", {"k": 0}, [1, 2, 3]):
            crc = zlib.crc32(py_compact(obj)) & 0xFFFFFFFF
            want = py_compact({"version": 1, "checksum": crc, "v1": obj})
            assert claimio.encode_checkpoint(obj, 1) == want


# ---------------------------------------------------------------------------
# atomicfile wiring
# ---------------------------------------------------------------------------


class TestAtomicfileWiring:
    @pytest.mark.parametrize(
        "obj", [{1: "a", 2: [1.5, None]}, {"s": 2.25, "t": float("inf")}, {"k": 1}]
    )
    def test_atomic_write_json_same_bytes_either_path(
        self, tmp_path, native_switch, obj
    ):
        native_switch(True)
        atomicfile.atomic_write_json(str(tmp_path / "n.json"), obj)
        native_switch(False)
        atomicfile.atomic_write_json(str(tmp_path / "p.json"), obj)
        want = py_compact(obj)
        assert (tmp_path / "n.json").read_bytes() == want
        assert (tmp_path / "p.json").read_bytes() == want

    def test_unsupported_through_atomic_write_json(self, tmp_path, native_switch):
        native_switch(True)
        with pytest.raises(TypeError):
            atomicfile.atomic_write_json(str(tmp_path / "x.json"), {"s": {1, 2}})
        with pytest.raises(TypeError):
            atomicfile.atomic_write_json(str(tmp_path / "x.json"), {"o": object()})
        assert os.listdir(tmp_path) == []

    def test_fallback_warns_once(self, tmp_path, native_switch, caplog, monkeypatch):
        monkeypatch.setattr(atomicfile, "_fallback_warned", False)
        native_switch(False)
        with caplog.at_level("WARNING", logger=atomicfile.__name__):
            atomicfile.atomic_write_text(str(tmp_path / "a"), "1")
            atomicfile.atomic_write_text(str(tmp_path / "b"), "2")
            atomicfile.atomic_write_json(str(tmp_path / "c"), {})
        hits = [r for r in caplog.records if "pure-Python path" in r.getMessage()]
        assert len(hits) == 1
        caplog.clear()
        native_switch(True)
        with caplog.at_level("WARNING", logger=atomicfile.__name__):
            atomicfile.atomic_write_text(str(tmp_path / "d"), "3")
        assert not caplog.records

    def test_deleted_parent_is_recreated(self, tmp_path, native_switch):
        native_switch(True)
        d = tmp_path / "sub" / "dir"
        target = str(d / "f.json")
        atomicfile.atomic_write_text(target, "one")
        shutil.rmtree(tmp_path / "sub")
        atomicfile.atomic_write_text(target, "two", durable=False)
        assert (d / "f.json").read_text() == "two"
        assert os.listdir(d) == ["f.json"]

    def test_threads_distinct_targets(self, tmp_path, native_switch):
        native_switch(True)
        d = tmp_path / "many"
        errors = []

        def worker(t):
            try:
                for i in range(200):
                    data = (f"{t}-{i}-" * (1 + (i % 50))).encode()
                    atomicfile.atomic_write_bytes(
                        str(d / f"t{t}-{i}.json"), data, durable=False
                    )
            except BaseException as e:  # surfaced below
                errors.append(e)

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors
        names = sorted(os.listdir(d))
        assert len(names) == 1600
        assert not [n for n in names if n.startswith(".tmp-")]
        for t in range(8):
            for i in range(200):
                want = (f"{t}-{i}-" * (1 + (i % 50))).encode()
                assert (d / f"t{t}-{i}.json").read_bytes() == want


# ---------------------------------------------------------------------------
# files written by the store and the CDI handler
# ---------------------------------------------------------------------------

SHARED_EDITS = ContainerEdits(
    env=[
        "AMD_DRA_CLAIM_UID=uid-x",
        "HSA_CU_MASK=0:0-63",
        "AMD_DRA_SHARED_SESSION=séssion",
    ],
    mounts=[
        Mount(host_path="/var/run/amd-dra/shm/uid-x", container_path="/dev/shm/amd-dra",
              options=["rw", "nosuid", "nodev", "bind"]),
    ],
)


def _write_both(tmp_path, native_switch, fn):
    """fn(root) writes under root and returns the file's path."""
    out = {}
    for label, on in (("native", True), ("python", False)):
        native_switch(on)
        root = tmp_path / label
        out[label] = open(fn(str(root)), "rb").read()
    native_switch(True)
    return out["native"], out["python"]


class TestFilesByteIdentical:
    @pytest.mark.parametrize("claim", CLAIMS, ids=["0dev", "1dev", "8dev"])
    def test_checkpoint_file(self, tmp_path, native_switch, claim):
        def write(root):
            store = CheckpointStore(root)
            store.write(claim)
            return store._path(claim.claim_uid)

        native, python = _write_both(tmp_path, native_switch, write)
        assert native == python
        v1 = claim.to_v1()
        assert native == py_compact(
            {"version": 1, "checksum": _checksum(v1), "v1": v1}
        )

    @pytest.mark.parametrize(
        "names,edits",
        [
            (["gpu-0"], ContainerEdits(env=["AMD_DRA_CLAIM_UID=uid-x"])),
            ([f"gpu-{i}" for i in range(8)], ContainerEdits(env=["AMD_DRA_CLAIM_UID=uid-x"])),
            (["gpu-0", "gpu-1-cpx-3"], SHARED_EDITS),
            ([], None),
        ],
        ids=["1dev", "8dev", "shared", "0dev"],
    )
    def test_claim_spec_file(self, tmp_path, native_switch, names, edits):
        def write(root):
            return CDIHandler(cdi_root=root).create_claim_spec("uid-x", names, edits)

        native, python = _write_both(tmp_path, native_switch, write)
        assert native == python
        json.loads(native)

    @pytest.mark.parametrize("read_native", [True, False], ids=["nread", "pyread"])
    @pytest.mark.parametrize("write_native", [True, False], ids=["nwrite", "pywrite"])
    def test_checkpoint_reads_back_across_paths(
        self, tmp_path, native_switch, write_native, read_native
    ):
        claim = CLAIMS[2]
        native_switch(write_native)
        CheckpointStore(str(tmp_path)).write(claim)
        native_switch(read_native)
        fresh = CheckpointStore(str(tmp_path))  # empty cache: disk read
        assert fresh._read_disk(claim.claim_uid) == claim
        assert fresh._read_disk("no-such-claim") is None
        assert fresh.read("no-such-claim") is None

    @pytest.mark.parametrize("read_native", [True, False], ids=["nread", "pyread"])
    def test_flipped_byte_is_corrupt(self, tmp_path, native_switch, read_native):
        claim = CLAIMS[1]
        native_switch(True)
        store = CheckpointStore(str(tmp_path))
        store.write(claim)
        path = store._path(claim.claim_uid)
        raw = bytearray(open(path, "rb").read())
        pos = raw.index(b'"gpu-0"') + 2  # inside a string value of the payload
        raw[pos] ^= 0x01
        with open(path, "wb") as f:
            f.write(raw)
        native_switch(read_native)
        with pytest.raises(CheckpointCorrupt):
            CheckpointStore(str(tmp_path))._read_disk(claim.claim_uid)
        # truncated (unparseable) files are corrupt too, not absent
        with open(path, "wb") as f:
            f.write(bytes(raw[: len(raw) // 2]))
        with pytest.raises(CheckpointCorrupt):
            CheckpointStore(str(tmp_path))._read_disk(claim.claim_uid)


# ---------------------------------------------------------------------------
# write_replace / read_or_none
# ---------------------------------------------------------------------------


class TestWriteReplace:
    @pytest.mark.parametrize("durable", [True, False])
    def test_success_leaves_no_temp(self, claimio, tmp_path, durable):
        tmp, path = str(tmp_path / ".tmp-1-0"), str(tmp_path / "f.json")
        claimio.write_replace(tmp, path, b"first", durable)
        claimio.write_replace(tmp, path, b"second", durable)
        assert os.listdir(tmp_path) == ["f.json"]
        assert open(path, "rb").read() == b"second"
        assert (os.stat(path).st_mode & 0o777) == (0o644 & ~_umask())

    def test_one_mib_payload(self, claimio, tmp_path):
        data = random.Random(1).randbytes(1 << 20)
        path = str(tmp_path / "big.bin")
        claimio.write_replace(str(tmp_path / ".tmp-1-1"), path, data, False)
        assert open(path, "rb").read() == data
        assert claimio.read_or_none(path) == data

    def test_rename_onto_nonempty_dir(self, claimio, tmp_path):
        target = tmp_path / "busy"
        target.mkdir()
        (target / "x").write_text("x")
        tmp = str(tmp_path / ".tmp-1-2")
        with pytest.raises(OSError) as ei:
            claimio.write_replace(tmp, str(target), b"data", False)
        assert ei.value.errno in (errno.EISDIR, errno.ENOTEMPTY, errno.EEXIST)
        assert ei.value.filename == str(target)
        assert sorted(os.listdir(tmp_path)) == ["busy"]

    def test_missing_parent_is_filenotfound_on_tmp(self, claimio, tmp_path):
        tmp = str(tmp_path / "gone" / ".tmp-1-3")
        with pytest.raises(FileNotFoundError) as ei:
            claimio.write_replace(tmp, str(tmp_path / "gone" / "f"), b"d", True)
        assert ei.value.errno == errno.ENOENT
        assert ei.value.filename == tmp

    def test_existing_tmp_is_not_clobbered(self, claimio, tmp_path):
        tmp = tmp_path / ".tmp-1-4"
        tmp.write_text("someone else's")
        with pytest.raises(FileExistsError):
            claimio.write_replace(str(tmp), str(tmp_path / "f"), b"d", False)
        assert tmp.read_text() == "someone else's"

    def test_data_must_be_bytes(self, claimio, tmp_path):
        with pytest.raises(TypeError):
            claimio.write_replace(
                str(tmp_path / ".tmp-1-5"), str(tmp_path / "f"), "text", False
            )
        assert os.listdir(tmp_path) == []


class TestReadOrNone:
    def test_missing_is_none(self, claimio, tmp_path):
        assert claimio.read_or_none(str(tmp_path / "nope")) is None
        assert claimio.read_or_none(str(tmp_path / "no" / "dir" / "f")) is None

    def test_exact_bytes(self, claimio, tmp_path):
        for data in (b"", b"x", b'{"a":1}\n', bytes(range(256)) * 100):
            p = tmp_path / "f.bin"
            p.write_bytes(data)
            assert claimio.read_or_none(str(p)) == data

    def test_other_errors_raise(self, claimio, tmp_path):
        with pytest.raises(IsADirectoryError) as ei:
            claimio.read_or_none(str(tmp_path))
        assert ei.value.filename == str(tmp_path)


def _umask() -> int:
    m = os.umask(0)
    os.umask(m)
    return m


# ---------------------------------------------------------------------------
# sanitizer run of the Python-free core (stand-alone program, CPU)
# ---------------------------------------------------------------------------


def test_core_selftest_under_asan_ubsan(tmp_path):
    from k8s_dra_driver_amd import build_native

    if build_native.sanitizer_link_flags() is None:
        pytest.skip("gcc has no ASan/UBSan runtime installed")
    exe = build_native.build_claimio_selftest(str(tmp_path / "claimio_selftest"))
    env = dict(os.environ, TMPDIR=str(tmp_path))
    out = subprocess.run(
        [exe], capture_output=True, text=True, env=env, timeout=120
    )
    assert out.returncode == 0, f"stdout:{out.stdout}\nstderr:{out.stderr[-3000:]}"
    assert "claimio_selftest: OK" in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
    assert os.listdir(tmp_path) == ["claimio_selftest"]

"""The HBM march self-test on an MI355X: ``hbm_fill``, ``hbm_march`` and
``hbm_verify`` and the host loop that drives them, through
``hbm_march_probe`` against the numpy reference, and the path from the child
process up to the driver at an explicit 1 GiB.

No test provokes a fault: what is injected is wrong data at word indices the
host has checked against the coverage before any launch, never a wrong
address. Every chunk comes back between canary guards and every test checks
them. No test uses the default coverage (all free memory): the machines are
shared.
"""

import numpy as np
import pytest

# torch must load before the system-ROCm-linked _hiphealth extension (see
# test_gpu.py): import order is load-bearing.
import torch  # noqa: F401

import hbmtest_reference as H
import hip_reference as R

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
TRIP = 256 * 16  # bytes one block covers per trip of its grid-stride loop


@pytest.fixture(scope="module")
def hh():
    from k8s_dra_driver_amd import _hiphealth

    assert _hiphealth.device_count() >= 1
    assert _hiphealth.PROBE_CANARY == R.CANARY
    assert _hiphealth.SELFTEST_MAX_RECORDS == H.MAX_RECORDS
    assert _hiphealth.HBMTEST_CHUNK_BYTES == H.CHUNK_BYTES
    assert _hiphealth.HBMTEST_PAGE_BYTES == H.PAGE_BYTES
    assert _hiphealth.HBMTEST_MIN_BYTES == H.MIN_BYTES
    assert _hiphealth.HBMTEST_RESERVE_MIN_BYTES == H.RESERVE_MIN_BYTES
    assert _hiphealth.HBMTEST_RESERVE_PERCENT == H.RESERVE_PERCENT
    return _hiphealth


def probe(hh, nbytes, rounds, blocks, chunk_bytes=None, flips=(), seed=SEED):
    """One probe call: ``(payload of every chunk, result, plan)``; the guards
    of every chunk are checked here."""
    chunk_bytes = chunk_bytes or nbytes
    raw, result = hh.hbm_march_probe(
        0, nbytes, seed, rounds, blocks, chunk_bytes, list(flips)
    )
    chunks = H.plan(nbytes, chunk_bytes)
    guard = hh.PROBE_GUARD_BYTES
    assert len(raw) == len(chunks)
    payloads = []
    for buf, (size, _) in zip(raw, chunks):
        assert len(buf) == size + 2 * guard
        canary = bytes([R.CANARY]) * guard
        assert buf[:guard] == canary and buf[guard + size :] == canary
        payloads.append(buf[guard : guard + size])
    assert result["bytes"] == nbytes and result["chunks"] == len(chunks)
    assert result["chunk_bytes"] == [size for size, _ in chunks]
    assert result["seed"] == seed and result["alloc_short"] is False
    return payloads, result, chunks


def assert_matches(result, payloads, want):
    """The parts of a result that the flips decide, against the reference."""
    for key in ("ok", "rounds", "passes", "mismatches", "flipped_or", "bad_pages"):
        assert result[key] == want[key], key
    assert [tuple(c) for c in result["bad_chunks"]] == want["bad_chunks"]
    assert [tuple(p) for p in result["bad_pages_first"]] == want["bad_pages_first"]
    records = [tuple(r) for r in result["records"]]
    assert len(records) == len(set(records)) == min(want["mismatches"], H.MAX_RECORDS)
    if want["mismatches"] <= H.MAX_RECORDS:
        assert set(records) == want["records"]
    else:
        assert set(records) <= want["records"]
    for c, (got, held) in enumerate(zip(payloads, want["contents"])):
        assert got == held, f"chunk {c}"


# ---------------------------------------------------------------------------
# clean runs
# ---------------------------------------------------------------------------
# around one trip of one block, around one trip of three blocks, and many
# trips with a tail
SIZES = [16, 4080, 4096, 4112, 3 * TRIP - 16, 3 * TRIP, 3 * TRIP + 16, (1 << 20) + 16]


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("nbytes", SIZES)
def test_a_clean_run_leaves_the_last_round_and_reports_nothing(hh, nbytes, blocks):
    # 1: fill and verify alone; 4: one cycle; 5 and 9: into a descending and
    # back into an ascending cycle, each with a seed of its own
    for rounds in (1, 4, 5, 9):
        payloads, result, chunks = probe(hh, nbytes, rounds, blocks)
        assert_matches(result, payloads, H.expected(SEED, rounds, chunks, []))
        assert result["ok"] is True and result["records"] == []
        assert (result["rounds"], result["passes"]) == (rounds, rounds + 1)
        assert payloads == H.contents(SEED, rounds - 1, chunks)


@pytest.mark.parametrize("blocks", [1, 3])
def test_the_word_index_runs_on_from_chunk_to_chunk(hh, blocks):
    """Three chunks of 4 KiB and a tail of 1 KiB: a kernel that starts w at 0
    in every chunk, or that mirrors n - 1 - i over another chunk's n, leaves
    other bytes than the reference at the chunk's global offset."""
    nbytes = 3 * 4096 + 1024
    for rounds in (1, 4, 5, 9):
        payloads, result, chunks = probe(hh, nbytes, rounds, blocks, chunk_bytes=4096)
        assert [c[1] for c in chunks] == [0, 512, 1024, 1536]
        assert result["ok"] is True and result["mismatches"] == 0
        whole = H.words(SEED, rounds - 1, 0, nbytes // 8).astype("<u8").tobytes()
        assert b"".join(payloads) == whole
        assert payloads[3] != payloads[0][:1024]


# ---------------------------------------------------------------------------
# injected flips
# ---------------------------------------------------------------------------
# (nbytes, chunk_bytes, blocks, words): the first and the last word, both
# sides of the border between chunk 0 and chunk 1, and both sides of a
# grid-stride boundary (element 255 | 256 with one block, 767 | 768 with
# three)
GEOMETRIES = {
    "chunks": (3 * 4096 + 1024, 4096, 1, [0, 511, 512, 1663]),
    "one-block": (3 * TRIP + 16, None, 1, [0, 511, 512, 1023, 1024, 1537]),
    "three-blocks": (3 * TRIP + 16, None, 3, [1, 1535, 1536, 1537]),
}
# of 9 rounds: pass 2 goes up, pass 5 comes down, pass 9 is the closing verify
PASSES = {"ascending": 2, "descending": 5, "verify": 9}


@pytest.mark.parametrize("pas", list(PASSES))
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_single_bit_flips_are_reported_where_and_when_they_are(hh, geometry, pas):
    nbytes, chunk_bytes, blocks, where = GEOMETRIES[geometry]
    rounds, p = 9, PASSES[pas]
    assert H.descending(p, rounds) == (pas == "descending")
    flips = [(p, w, 1 << ((7 * i + 3) % 64)) for i, w in enumerate(where)]
    flips.append((p, where[0], 1 << 63))  # two bits of one word: one record
    payloads, result, chunks = probe(hh, nbytes, rounds, blocks, chunk_bytes, flips)
    want = H.expected(SEED, rounds, chunks, flips)
    assert want["mismatches"] == len(where) and want["passes"] == p + 1
    assert_matches(result, payloads, want)
    assert result["ok"] is False
    for r in result["records"]:
        assert r[0] == p and r[3] == H.word(SEED, p - 1, r[1])
    if pas == "verify":  # the flipped words stay as they were read
        assert payloads != H.contents(SEED, rounds - 1, chunks)
    else:  # the march wrote round p over them, and no later pass ran
        assert payloads == H.contents(SEED, p, chunks)


def test_a_flip_in_a_later_pass_never_happens_after_a_bad_pass(hh):
    nbytes = 3 * 4096 + 1024
    flips = [(3, 600, 1 << 40), (6, 0, 1)]
    payloads, result, chunks = probe(hh, nbytes, 9, 1, 4096, flips)
    assert_matches(result, payloads, H.expected(SEED, 9, chunks, flips))
    want = H.word(SEED, 2, 600)
    assert [tuple(r) for r in result["records"]] == [(3, 600, want ^ (1 << 40), want)]
    assert (result["passes"], result["rounds"]) == (4, 4)
    assert [tuple(c) for c in result["bad_chunks"]] == [(1, 1)]


def test_masks_that_cancel_are_no_mismatch(hh):
    flips = [(2, 5, 1), (2, 5, 1)]
    payloads, result, chunks = probe(hh, 4096, 4, 1, flips=flips)
    assert result["ok"] is True and result["passes"] == 5
    assert payloads == H.contents(SEED, 3, chunks)


def test_bad_pages_are_counted_inside_their_chunk(hh):
    """Two chunks of 2 MiB + 4 KiB: each has a page 0 and the start of a
    page 1."""
    chunk_bytes = H.PAGE_BYTES + 4096
    nbytes = 2 * chunk_bytes
    w1 = chunk_bytes // 8
    page1 = H.PAGE_BYTES // 8
    flips = [
        (1, 0, 1), (1, page1 - 1, 2),  # chunk 0 page 0, twice
        (1, w1 + page1, 4), (1, w1 + page1 + 511, 8),  # chunk 1 page 1, twice
        (1, w1 + page1 - 1, 16),  # chunk 1 page 0
    ]
    payloads, result, chunks = probe(hh, nbytes, 4, 3, chunk_bytes, flips)
    want = H.expected(SEED, 4, chunks, flips)
    assert want["bad_pages_first"] == [(0, 0), (1, 0), (1, 1)]
    assert want["bad_chunks"] == [(0, 2), (1, 3)] and want["flipped_or"] == 31
    assert_matches(result, payloads, want)


def test_100_flips_in_one_pass_are_counted_exactly_with_64_records(hh):
    nbytes = 3 * TRIP + 16
    rng = np.random.default_rng(5)
    where = rng.choice(nbytes // 8, size=100, replace=False).tolist()
    flips = [(6, w, 1 << (i % 64)) for i, w in enumerate(where)]
    payloads, result, chunks = probe(hh, nbytes, 8, 3, flips=flips)
    want = H.expected(SEED, 8, chunks, flips)
    assert want["mismatches"] == 100 and len(want["records"]) == 100
    assert_matches(result, payloads, want)
    assert result["mismatches"] == 100 and len(result["records"]) == 64
    assert len({r[1] for r in result["records"]}) == 64
    assert result["flipped_or"] == 2**64 - 1


# ---------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------
@pytest.mark.parametrize(
    "kw",
    [
        dict(flips=[(1, 512, 1)]),  # the first word past the coverage
        dict(flips=[(1, -1, 1)]),
        dict(flips=[(1, 2**40, 1)]),
        dict(flips=[(0, 0, 1)]),  # pass 0 reads nothing
        dict(flips=[(5, 0, 1)]),  # rounds is 4
        dict(flips=[(-1, 0, 1)]),
        dict(nbytes=4104),  # not a multiple of 16
        dict(nbytes=0),
        dict(nbytes=(64 << 20) + 16),  # over the probe's cap
        dict(chunk_bytes=24),
        dict(chunk_bytes=0),
        dict(nbytes=4096, chunk_bytes=16),  # more chunks than the probe takes
        dict(rounds=0),
        dict(rounds=65),
        dict(blocks=0),
        dict(blocks=4097),
        dict(device=-1),
        dict(device=4096),
    ],
)
def test_arguments_are_refused_before_any_launch(hh, kw):
    args = dict(device=0, nbytes=4096, seed=SEED, rounds=4, blocks=1,
                chunk_bytes=4096, flips=[])
    args.update(kw)
    with pytest.raises(ValueError):
        hh.hbm_march_probe(**args)


@pytest.mark.parametrize(
    "kw",
    [dict(seconds=0), dict(seconds=-1), dict(seconds=601), dict(mib=512),
     dict(mib=-1), dict(mib=(1 << 18) + 1), dict(blocks=-1), dict(blocks=4097),
     dict(device=-1)],
)
def test_the_production_call_refuses_its_arguments_too(hh, kw):
    args = dict(device=0, seconds=1.0, mib=1024)
    args.update(kw)
    with pytest.raises(ValueError):
        hh.hbm_selftest(**args)


# ---------------------------------------------------------------------------
# production path, at an explicit 1 GiB
# ---------------------------------------------------------------------------
def test_one_second_over_one_gib(hh):
    r = hh.hbm_selftest(0, seconds=1, mib=1024)
    print(
        f"hbm_selftest 1 GiB: {r['passes']} passes in {r['seconds']:.2f}s "
        f"(allocation {r['alloc_seconds']:.2f}s), GB/s {r['gbs']}, "
        f"free {r['free_bytes'] >> 20} of {r['total_bytes'] >> 20} MiB"
    )
    assert r["ok"] is True and r["mismatches"] == 0 and r["flipped_or"] == 0
    assert r["records"] == [] and r["bad_chunks"] == [] and r["bad_pages"] == 0
    assert r["bad_pages_first"] == []
    assert r["bytes"] == 2**30 and r["chunks"] == 1 and r["chunk_bytes"] == [2**30]
    assert r["alloc_short"] is False
    assert r["rounds"] >= 4 and r["rounds"] % 4 == 0
    assert r["passes"] == r["rounds"] + 1
    assert r["seconds"] >= 1.0
    assert 0 < r["free_bytes"] <= r["total_bytes"]
    assert sorted(r["gbs"]) == ["fill", "march_addr", "march_hash", "verify"]
    assert all(v > 0 for v in r["gbs"].values())


@pytest.fixture(scope="module")
def real_lib():
    from k8s_dra_driver_amd.hal.amdsmi import AmdSmiDeviceLib

    lib = AmdSmiDeviceLib()
    lib.open()
    yield lib
    lib.close()


def test_the_child_passes_with_the_march(hh, real_lib):
    from k8s_dra_driver_amd import selftest

    gpu = real_lib.enumerate()[0]
    res = selftest.run(gpu, mib=64, hbm_seconds=1, hbm_mib=1024)
    print("child --hbm-seconds 1 --hbm-mib 1024:", res.outcome,
          f"{res.seconds:.2f}s", res.error)
    assert res.outcome == "pass", res.error
    assert res.findings() == []
    hbm = res.report["hbm"]
    assert hbm["ok"] is True and hbm["bytes"] == 2**30
    assert hbm["rounds"] % 4 == 0 and hbm["passes"] == hbm["rounds"] + 1
    assert hbm["mismatches"] == 0


def test_driver_startup_selftest_with_the_march_on_the_real_hal(real_lib, tmp_path):
    from k8s_dra_driver_amd.kube.client import InMemoryKube
    from k8s_dra_driver_amd.plugin.driver import Driver

    kube = InMemoryKube()
    kube.api_versions = ["v1beta2", "v1beta1"]
    driver = Driver(
        real_lib,
        kube,
        node_name="gpu-node",
        cdi_root=str(tmp_path / "cdi"),
        checkpoint_root=str(tmp_path / "state"),
        use_tmpfs=False,
        gpu_indices=[0],
    )
    try:
        results = driver.run_startup_selftest(mib=64, hbm_seconds=1, hbm_mib=1024)
        assert results == {0: "pass"}
        assert driver.health.findings(0) == []
        value = driver.metrics.registry.get_sample_value
        assert value("dra_gpu_selftest_hbm_bytes", {"gpu": "0"}) == 2**30
        assert value("dra_gpu_selftest_hbm_passes", {"gpu": "0"}) >= 5
        assert value("dra_gpu_selftest_hbm_mismatches", {"gpu": "0"}) == 0
    finally:
        driver.shutdown(unpublish=False)

"""Health policy: evaluate(baseline, previous, current) -> findings.

Table-driven: one case per row of the policy table (docs/operations.md)
plus the boundaries of every comparison.
"""

import dataclasses

import pytest

from k8s_dra_driver_amd.hal.model import HEALTH_SIGNAL_NAMES, HealthSignals
from k8s_dra_driver_amd.plugin.health import HealthFinding, evaluate


def clean(**over) -> HealthSignals:
    base = dict(
        ecc_correctable=0,
        ecc_uncorrectable=0,
        ecc_deferred=0,
        ecc_blocks={},
        bad_pages_reserved=0,
        bad_pages_pending=0,
        bad_pages_unreservable=0,
        bad_page_threshold=128,
        temp_hotspot_c=50.0,
        temp_hotspot_crit_c=110.0,
        temp_vram_c=45.0,
        temp_vram_crit_c=105.0,
        throttle_prochot=False,
        throttle_ppt=False,
        throttle_socket_thermal=False,
        throttle_vr_thermal=False,
        throttle_hbm_thermal=False,
    )
    base.update(over)
    return HealthSignals(**base)


# (id, baseline overrides, previous overrides, current overrides,
#  expected [(reason, severity)])
CASES = [
    ("clean", {}, {}, {}, []),
    # -- uncorrectable ECC --------------------------------------------
    (
        "ue_above_baseline",
        {},
        {},
        {"ecc_uncorrectable": 1},
        [("UncorrectableEcc", "fatal")],
    ),
    (
        "ue_above_nonzero_baseline",
        {"ecc_uncorrectable": 4},
        {"ecc_uncorrectable": 4},
        {"ecc_uncorrectable": 5},
        [("UncorrectableEcc", "fatal")],
    ),
    (
        "ue_equal_to_baseline_zero",
        {"ecc_uncorrectable": 0},
        {},
        {"ecc_uncorrectable": 0},
        [],
    ),
    (
        "ue_equal_to_nonzero_baseline_is_historic_only",
        {"ecc_uncorrectable": 4},
        {"ecc_uncorrectable": 4},
        {"ecc_uncorrectable": 4},
        [("UncorrectableEccHistoric", "warning")],
    ),
    # -- retired pages -------------------------------------------------
    (
        "page_pending",
        {},
        {},
        {"bad_pages_pending": 1},
        [("BadPagesPending", "fatal")],
    ),
    (
        "page_unreservable",
        {},
        {},
        {"bad_pages_unreservable": 1},
        [("BadPageUnreservable", "fatal")],
    ),
    (
        "reserved_equal_to_threshold",
        {},
        {},
        {"bad_pages_reserved": 128, "bad_page_threshold": 128},
        [("BadPageThreshold", "fatal")],
    ),
    (
        "reserved_above_threshold",
        {},
        {},
        {"bad_pages_reserved": 200, "bad_page_threshold": 128},
        [("BadPageThreshold", "fatal")],
    ),
    (
        "reserved_one_below_threshold",
        {},
        {},
        {"bad_pages_reserved": 127, "bad_page_threshold": 128},
        [("RetiredPages", "warning")],
    ),
    (
        "threshold_zero_never_fatal",
        {},
        {},
        {"bad_pages_reserved": 500, "bad_page_threshold": 0},
        [("RetiredPages", "warning")],
    ),
    (
        "threshold_none_never_fatal",
        {},
        {},
        {"bad_pages_reserved": 500, "bad_page_threshold": None},
        [("RetiredPages", "warning")],
    ),
    (
        "no_reserved_pages_with_threshold_zero",
        {},
        {},
        {"bad_pages_reserved": 0, "bad_page_threshold": 0},
        [],
    ),
    # -- thermal -------------------------------------------------------
    (
        "hotspot_equal_to_critical",
        {},
        {},
        {"temp_hotspot_c": 110.0},
        [("ThermalCritical", "soft")],
    ),
    (
        "hotspot_just_below_critical",
        {},
        {},
        {"temp_hotspot_c": 109.0},
        [],
    ),
    (
        "vram_above_critical",
        {},
        {},
        {"temp_vram_c": 106.0},
        [("ThermalCritical", "soft")],
    ),
    (
        "both_sensors_critical_is_one_finding",
        {},
        {},
        {"temp_hotspot_c": 111.0, "temp_vram_c": 106.0},
        [("ThermalCritical", "soft")],
    ),
    (
        "critical_limit_zero_is_not_a_limit",
        {},
        {},
        {"temp_hotspot_c": 60.0, "temp_hotspot_crit_c": 0},
        [],
    ),
    (
        "critical_limit_unsupported",
        {},
        {},
        {"temp_hotspot_c": 200.0, "temp_hotspot_crit_c": None},
        [],
    ),
    # -- warnings ------------------------------------------------------
    (
        "correctable_growth",
        {},
        {"ecc_correctable": 10},
        {"ecc_correctable": 11},
        [("CorrectableEccGrowth", "warning")],
    ),
    (
        "correctable_steady",
        {},
        {"ecc_correctable": 10},
        {"ecc_correctable": 10},
        [],
    ),
    (
        "deferred_growth",
        {},
        {"ecc_deferred": 0},
        {"ecc_deferred": 2},
        [("DeferredEcc", "warning")],
    ),
    (
        "throttled",
        {},
        {},
        {"throttle_ppt": True},
        [("Throttled", "warning")],
    ),
    # -- ordering: fatal, soft, warning; table order within a class ----
    (
        "everything_at_once",
        {},
        {},
        {
            "ecc_uncorrectable": 2,
            "ecc_correctable": 7,
            "bad_pages_pending": 1,
            "bad_pages_unreservable": 1,
            "bad_pages_reserved": 128,
            "temp_vram_c": 105.0,
            "throttle_hbm_thermal": True,
        },
        [
            ("UncorrectableEcc", "fatal"),
            ("BadPagesPending", "fatal"),
            ("BadPageUnreservable", "fatal"),
            ("BadPageThreshold", "fatal"),
            ("ThermalCritical", "soft"),
            ("CorrectableEccGrowth", "warning"),
            ("Throttled", "warning"),
        ],
    ),
]


@pytest.mark.parametrize(
    "base,prev,cur,expected",
    [c[1:] for c in CASES],
    ids=[c[0] for c in CASES],
)
def test_policy_table(base, prev, cur, expected):
    found = evaluate(clean(**base), clean(**prev), clean(**cur))
    assert [(f.reason, f.severity) for f in found] == expected
    assert all(isinstance(f, HealthFinding) and f.detail for f in found)


def test_all_none_signals_yield_nothing():
    nothing = HealthSignals()
    assert all(getattr(nothing, n) is None for n in HEALTH_SIGNAL_NAMES)
    assert evaluate(nothing, nothing, nothing) == []
    assert evaluate(None, None, nothing) == []
    # unsupported on one side of a comparison only: still no finding
    assert evaluate(nothing, nothing, clean()) == []
    assert evaluate(clean(), clean(ecc_correctable=3), nothing) == []


def test_all_unsupported_lists_every_signal():
    s = HealthSignals.all_unsupported("nope")
    assert set(s.unsupported) == set(HEALTH_SIGNAL_NAMES)
    assert evaluate(s, s, s) == []


def test_first_poll_has_no_previous():
    # growth warnings need a previous reading; fatal rows do not
    cur = clean(ecc_correctable=9, bad_pages_pending=2)
    found = evaluate(cur, None, cur)
    assert [f.reason for f in found] == ["BadPagesPending"]


def test_evaluate_is_pure():
    base, prev, cur = clean(), clean(), clean(ecc_uncorrectable=3)
    before = [dataclasses.asdict(s) for s in (base, prev, cur)]
    evaluate(base, prev, cur)
    assert [dataclasses.asdict(s) for s in (base, prev, cur)] == before

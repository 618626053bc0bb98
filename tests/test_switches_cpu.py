"""CPU-only: the table of environment switches (hyphy_amd/csrc/switches.h, hyphy_hip_plan_switches).  Structure: one place calls
getenv, every name in the sources is a row, the documents follow the table, the read times are what they were.  Parsing: every
primitive on the values that tell it from its neighbours, through a fresh read of the environment in this process."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hyphy_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hyphy_hip.h")
TOKEN = re.compile(r"HYPHY_HIP_([A-Z0-9_]+)")
# the adapter's own variables (integration/, hyphy_amd/hip.py): not the library's, not in the table
ADAPTER = {"DEVICE", "DEVICES", "WORLD", "RANK", "LOCAL_RANK", "RUN_ID", "UID_FILE", "COLLECTIVE", "DEVICE_EXPM", "TEMPLATES", "MIXTURES",
           "CAT_BATCH", "MIN_PATTERNS", "DEBUG", "KEEP_PATCHED", "LIB", "JOINT", "MARGINAL"}
HEADER_MACROS = {"H", "OWN_STREAM"}  # (what include/hyphy_hip.h #defines)
# the ten names subtree repeats used to walk by hand before they gave way to a forced per-pattern form
PER_PATTERN = ["KERNEL", "WAVE_VARIANT", "CUT", "CHAIN_M", "FRAGMENT", "SLOTS", "REROOT", "TILES", "TIMELINE", "ABLATE"]
PREDICATES = ["per_pattern_forced", "schedule_forced", "wave_form_forced"]


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    from hyphy_amd import hip
    return hip


@pytest.fixture
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("HYPHY_HIP_") and k[len("HYPHY_HIP_"):] not in ADAPTER:
            monkeypatch.delenv(k)
    return monkeypatch


def _rows(hip):
    return {r["name"]: r for r in hip.plan_switches()}


def _value(hip, name):
    return _rows(hip)[name]["value"]


def _set(mp, name, value):
    if value is None:
        mp.delenv("HYPHY_HIP_" + name, raising=False)
    else:
        mp.setenv("HYPHY_HIP_" + name, value)


# ---- structure ---------------------------------------------------------------------------------------------------------------

def test_one_file_calls_getenv():
    holders = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(f) and "getenv" in open(f).read()]
    assert holders == ["switches.h"]


def test_no_switch_name_is_passed_as_a_string_outside_the_table():
    for f in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        if os.path.basename(f) != "switches.h":
            assert '"HYPHY_HIP_' not in open(f).read(), f


def test_rows_are_well_formed(hip):
    rows = hip.plan_switches()
    names = [r["name"] for r in rows]
    assert len(names) == len(set(names))
    for r in rows:
        assert set(r) == {"name", "kind", "when", "audience", "default", "value"}, r
        assert r["when"] in ("process", "create", "call"), r
        assert r["audience"] in ("integrator", "diagnostic"), r
    assert [r["name"] for r in rows if r["kind"] == "predicate"] == PREDICATES
    assert [r["name"] for r in rows if r["kind"] == "prefix"] == ["NOPOISON_"]


def test_every_name_in_the_sources_is_a_row(hip):
    rows = set(_rows(hip))
    for f in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + [HEADER]:
        for name in TOKEN.findall(open(f).read()):
            assert name in rows or name in ADAPTER or name in HEADER_MACROS, (os.path.basename(f), name)


def test_every_row_is_on_the_switches_page(hip):
    page = open(os.path.join(ROOT, "docs", "switches.md")).read()
    for r in hip.plan_switches():
        assert ("HYPHY_HIP_" + r["name"] if r["kind"] != "predicate" else r["name"]) in page, r["name"]
    # whole names, not prefixes of longer ones
    on_page = set(TOKEN.findall(page))
    assert {r["name"] for r in hip.plan_switches() if r["kind"] != "predicate"} <= on_page
    assert on_page - set(_rows(hip)) <= ADAPTER


def test_header_lists_exactly_the_integrator_rows(hip):
    txt = open(HEADER).read()
    block = txt[txt.index("Environment switches."):txt.index("Everything else that starts with HYPHY_HIP_")]
    assert set(TOKEN.findall(block)) == {r["name"] for r in hip.plan_switches() if r["audience"] == "integrator"}
    assert not re.search(r"\bTEN\b|about forty", txt)


def test_read_times_are_the_parents(hip):
    """What a `static const` held at the sites this table replaced is `process`, nothing else is.  The eleven names the sites
    `static const ... getenv` gave (two of the thirteen sites were second reads, of TUNE_CACHE and REDUCE) — and POOL_MB, whose
    static const sat in front of a lambda (pool.hip cap_bytes): it was read once per process too, and stays so."""
    process = {r["name"] for r in hip.plan_switches() if r["when"] == "process"}
    assert process == {"SPIN", "EXPM_MASK", "TIMING_EVERY", "EXPM_PROF", "TUNE_CACHE", "TEAM", "COEF_INLINE", "EXPM", "EXPM_DEGREE", "NUC", "REDUCE",
                       "POOL_MB"}
    rows = _rows(hip)
    for name in ("SITE_EXPORT", "TRUNK_TEAM", "XCD_PAD"):  # the tests run both forms in one process
        assert rows[name]["when"] == "call", name
    for name in ("ALL_TIMINGS", "REPEATS", "CACHE", "KERNEL"):
        assert rows[name]["when"] == "create", name


def test_size_query_and_short_buffer(hip):
    import ctypes
    lib = hip.load()
    need = -lib.hyphy_hip_plan_switches(None, 0)
    assert need > 1000
    buf = ctypes.create_string_buffer(need)
    assert lib.hyphy_hip_plan_switches(buf, need - 1) == -need and buf.value == b""
    assert lib.hyphy_hip_plan_switches(buf, need) == need and len(buf.value) == need - 1


# ---- parsing, by primitive: atoi / atof as the library has always applied them ----------------------------------------------------

@pytest.mark.parametrize("name", ["TUNE", "XCD_PAD"])
def test_on_unless_zero(hip, clean_env, name):
    assert _value(hip, name) == "on"
    for v in ("0", "00", " 0", "", "abc"):
        _set(clean_env, name, v)
        assert _value(hip, name) == "off", repr(v)
    for v in ("1", "2", "-1", "1x"):
        _set(clean_env, name, v)
        assert _value(hip, name) == "on", repr(v)


def test_present(hip, clean_env):
    assert _value(hip, "POISON") == "off"
    for v in ("", "0", "1"):
        _set(clean_env, "POISON", v)
        assert _value(hip, "POISON") == "on", repr(v)


def test_verbose_keeps_both_parsers(hip, clean_env):
    assert _value(hip, "VERBOSE") == "off"
    for v, want in (("1", "on,1"), ("2", "on,2"), ("", "on,0")):
        _set(clean_env, "VERBOSE", v)
        assert _value(hip, "VERBOSE") == want


def test_integers_and_their_clamps(hip, clean_env):
    for name, cases in {"TIMING_EVERY": [(None, "16"), ("0", "1"), ("5", "5"), ("x", "1")],
                        "SLOTS": [("9", "4"), ("1", "2"), ("3", "3")],
                        "KERNEL": [("7", "2"), ("-3", "0")],
                        "NUCGEN_AFTER": [(None, "8"), ("0", "1")],
                        "CHAIN_M": [("0", "1"), ("12", "12")]}.items():
        for v, want in cases:
            _set(clean_env, name, v)
            assert _value(hip, name) == want, (name, v)


def test_forced_either_way_or_left_to_the_library(hip, clean_env):
    assert _value(hip, "FUSED_REDUCE") == "auto"
    for v, want in (("0", "off"), ("", "off"), ("1", "on"), ("-1", "on")):
        _set(clean_env, "FUSED_REDUCE", v)
        assert _value(hip, "FUSED_REDUCE") == want


def test_reals(hip, clean_env):
    for v, want in (("0.3", "0.3"), ("x", "0"), ("1e-2", "0.01")):
        _set(clean_env, "REP_THETA", v)
        assert _value(hip, "REP_THETA") == want
    assert _value(hip, "EXCHANGE_TIMEOUT_S") == "120"
    _set(clean_env, "EXCHANGE_TIMEOUT_S", "soon")  # (malformed: 0 seconds, as it has always been)
    assert _value(hip, "EXCHANGE_TIMEOUT_S") == "0"


def test_megabytes(hip, clean_env):
    for v in (None, "0", "-3", "x"):
        _set(clean_env, "TRIALS_MB", v)
        assert _value(hip, "TRIALS_MB") == str(1024 << 20), repr(v)
    _set(clean_env, "TRIALS_MB", "0.5")
    assert _value(hip, "TRIALS_MB") == "524288"
    for v, want in ((None, 1024 << 20), ("0", 0), ("-5", 0), ("2", 2 << 20), ("0.5", 0)):  # POOL_MB: atol, negative is off
        _set(clean_env, "POOL_MB", v)
        assert _value(hip, "POOL_MB") == str(want), repr(v)
    _set(clean_env, "REP_MAX_MB", "-1")
    assert _value(hip, "REP_MAX_MB") == "0"
    _set(clean_env, "REP_MAX_MB", "3")
    assert _value(hip, "REP_MAX_MB") == str(3 << 20)


def test_words(hip, clean_env):
    for name, cases in {"CACHE": [(None, "lazy"), ("always", "always"), ("Always", "lazy"), ("", "lazy"), ("1", "lazy")],
                        "CUT": [("levels", "levels"), ("chains", "chains"), ("level", "chains")],
                        "REDUCE": [(None, "auto"), ("block", "block"), ("wave", "wave"), ("x", "auto"), ("block|wave", "auto")],
                        "COMBINE": [(None, "host"), ("rccl", "rccl"), ("nccl", "host")]}.items():
        for v, want in cases:
            _set(clean_env, name, v)
            assert _value(hip, name) == want, (name, v)


def test_paths(hip, clean_env):
    assert _value(hip, "TIMELINE") == "-"
    _set(clean_env, "TIMELINE", "/tmp/a b.txt")
    assert _value(hip, "TIMELINE") == "/tmp/a b.txt"


def test_predicates(hip, clean_env):
    def preds():
        rows = _rows(hip)
        return tuple(rows[n]["value"] == "on" for n in PREDICATES)
    assert preds() == (False, False, False)
    for name in PER_PATTERN:
        _set(clean_env, name, "")  # (given at all: any value)
        assert preds()[0], name
        _set(clean_env, name, None)
    _set(clean_env, "REPEATS", "1")
    assert preds() == (False, False, False)
    _set(clean_env, "REPEATS", None)
    for name in ("CHAIN_M", "CUT", "FRAGMENT"):
        _set(clean_env, name, "0")
        assert preds()[1], name
        _set(clean_env, name, None)
    for name in sorted(set(PER_PATTERN) - {"CHAIN_M", "CUT", "FRAGMENT"}):
        _set(clean_env, name, "1")
        assert not preds()[1], name
        _set(clean_env, name, None)
    _set(clean_env, "WAVE_VARIANT", "2")
    assert preds() == (True, False, True)
    _set(clean_env, "WAVE_VARIANT", None)
    _set(clean_env, "SLOTS", "3")
    assert preds() == (True, False, True)
    _set(clean_env, "SLOTS", None)
    _set(clean_env, "REROOT", "1")  # (the tuner asks for REROOT by itself)
    assert preds() == (True, False, False)

"""The measurement switches of HS_DEBUG_FLAGS: one table (hyperslam_amd/csrc/switches.hpp), read by the C++ code as an X-macro and by
hyperslam_amd/switches.py as text. The values are frozen — bench.py, profiles/ and the documents quote them — and no source file of the
library may test a switch by its number."""
import glob
import os
import re

from hyperslam_amd import switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# value -> what it selects, as the documents quote it. 8192 has two names: the only shared bit.
FROZEN = {
    1: "skip the backward sweep", 2: "skip the rank-6 updates", 4: "pre-look-ahead factorisation", 8: "no k_dense_solve_mx on small systems",
    16: "phase stamps, factorisation and sweeps", 32: "per-workgroup stamps, linearise / gram / build", 64: "two-ended on k_band_factor_la",
    128: "border sweep behind the factorisation", 256: "stamps of k_assemble", 512: "stamps of k_update_visual", 1024: "no k_gram_pair",
    2048: "one-ended factorisation", 4096: "k_finalize_reduced in every iteration", 8192: "two meanings",
    16384: "join by events instead of device flags", 32768: "k_pack_decision behind every update", 65536: "k_band_backward_w",
    131072: "k_band_factor_mfma", 262144: "do not decouple leading constant rows", 524288: "border Cholesky in LDS",
    1048576: "inertial branch on the main stream", 2097152: "banded kernels instead of k_dense_factor", 4194304: "k_landmark<K,4,1>",
    8388608: "five finalisation launches", 16777216: "k_commit launch for small windows", 33554432: "one cost launch per factor type",
    67108864: "k_commit in every iteration", 134217728: "prior / inertial candidate costs as own launches",
    268435456: "backward sweeps one block row per step", 536870912: "bordered systems one-ended", 1073741824: "no speculative linearisation",
    4294967296: "k_band_backward_sb (two phases)",
}
SHARED = {8192: {"border_solve_reg", "backward2_one_ended"}}


def test_table_equals_the_frozen_values():
    by_value = {}
    for name, bit, meaning in switches.TABLE:
        assert meaning.strip(), name
        by_value.setdefault(1 << bit, set()).add(name)
    assert sorted(by_value) == sorted(FROZEN)
    assert {v: n for v, n in by_value.items() if len(n) > 1} == SHARED  # bits are unique but for the one documented pair
    assert "shares bit 13" in switches.MEANINGS["backward2_one_ended"]  # ... which the table states in words
    names = [name for name, _, _ in switches.TABLE]
    assert len(names) == len(set(names)) == len(FROZEN) + 1
    assert switches.VALUES == {name: 1 << bit for name, bit, _ in switches.TABLE}


def test_header_holds_nothing_but_the_table_lines():
    """Every HS_SWITCH( of the header outside the X-macro's own definition is a line the regular expression takes: none is lost to a format it
    does not know."""
    with open(switches.HEADER) as f:
        text = f.read()
    rows = [ln for ln in text.splitlines() if re.match(r"\s*HS_SWITCH\(\s*\w+\s*,\s*\d", ln)]
    assert len(rows) == len(switches.TABLE) == 33


def test_names_and_numbers_round_trip(monkeypatch):
    assert switches.flags() == "0" and switches.names(0) == []
    for name, value in switches.VALUES.items():
        assert int(switches.flags(name)) == value and name in switches.names(value)
    both = switches.flags("backward_sb", "one_ended")  # the switch of the second word with one of the first
    assert both == str(4294967296 + 2048) and switches.names(both) == ["one_ended", "backward_sb"]
    every = switches.value(*switches.VALUES)
    assert every == sum(FROZEN) and switches.names(every) == [name for name, _, _ in switches.TABLE]
    assert switches.names(8192) == ["border_solve_reg", "backward2_one_ended"]
    monkeypatch.setenv("HS_DEBUG_FLAGS", "2048")
    assert switches.add_to_env("backward_sb", "stamp_factor") == 4294967296 + 2048 + 16 and os.environ["HS_DEBUG_FLAGS"] == "4294969360"


def test_no_switch_is_tested_by_its_number():
    """hyperslam_amd/csrc/*.hpp, capi.hip and tools/ab/*.hpp (which the profiling build includes): no decimal literal as the second operand of
    `debug_flags &`, `debug_flags2 &`, HS_AB( .. , or prof_enabled( .. , ."""
    files = sorted(glob.glob(os.path.join(ROOT, "hyperslam_amd", "csrc", "*.hpp"))) + [os.path.join(ROOT, "hyperslam_amd", "csrc", "capi.hip")] + \
        sorted(glob.glob(os.path.join(ROOT, "tools", "ab", "*.hpp")))
    assert len(files) > 25 and any(f.endswith("kernels_backward2.hpp") for f in files)
    numeral = re.compile(r"debug_flags2?\s*&\s*\(?\s*\d|(?:HS_AB|prof_enabled)\s*\([^,()]*,\s*\(?\s*\d")
    found = []
    for path in files:
        with open(path) as f:
            for no, line in enumerate(f, 1):
                if numeral.search(line):
                    found.append("%s:%d: %s" % (os.path.relpath(path, ROOT), no, line.strip()))
    assert not found, "\n".join(found)
    assert numeral.search("if (T.debug_flags & 2048) x;") and numeral.search("HS_AB(T.debug_flags, 131072)") and \
        numeral.search("prof_enabled(T.debug_flags, 16)") and numeral.search("!(T.debug_flags2 & 1)")  # (the expression finds what it is for)

"""The library's environment switches: every ALVA_* name it reads is documented in README's table, and the retired A/B switches
(with the code paths only they reached) stay gone.  The check runs from the library to the table only: the table also lists
build-time and Python-side names."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "alvaar_amd"
SOURCES = (".hip", ".hpp", ".cpp", ".h", ".inc", ".py")

RETIRED = ("ALVA_TRACK_LISTS", "ALVA_ORB_SIDE_BLUR", "ALVA_TRACK_KLT_LANES", "ALVA_LANE_KLT_LANES", "ALVA_P3P_NO_INLINE_SAMPLES",
           "ALVA_LANE_SEGMENTS", "ALVA_LANE_XCD", "ALVA_PYR_T1", "ALVA_PYR_T2", "ALVA_PYR_T3", "ALVA_BAR_FLAG", "ALVA_PYRAMID_STAGES",
           "ALVA_BA_HOST_LM")


def _sources():
    return [p for p in sorted(PKG.rglob("*")) if p.is_file() and p.suffix in SOURCES]


def _names_read():
    names = set()
    for p in sorted((PKG / "csrc").rglob("*")):
        if p.is_file() and p.suffix in SOURCES:
            names.update(re.findall(r'getenv\(\s*"(ALVA_[A-Z0-9_]+)"', p.read_text()))
    for p in sorted(PKG.glob("*.py")):
        names.update(re.findall(r'os\.environ(?:\.get)?\s*[(\[]\s*["\'](ALVA_[A-Z0-9_]+)', p.read_text()))
    return names


def test_every_switch_the_library_reads_is_in_the_readme_table():
    names = _names_read()
    assert len(names) > 20, sorted(names)   # the scan itself works
    table = set()
    for line in (ROOT / "README.md").read_text().splitlines():
        if line.startswith("| `"):
            table.update(re.findall(r"ALVA_[A-Z0-9_]+", line.split(" | ")[0]))
    assert not names - table, f"undocumented switches: {sorted(names - table)}"


def test_retired_switches_stay_retired():
    found = [(str(p.relative_to(ROOT)), n) for p in _sources() for n in RETIRED if re.search(n + r"(?![A-Z0-9_])", p.read_text())]
    assert not found, found

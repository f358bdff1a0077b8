"""The run-time switches of the library live in one header, csrc/spp_switches.h, and are listed for users in the table of
tools/README.md: the two name the same switches, and no other file under csrc/ reads the environment."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")
HEADER = os.path.join(CSRC, "spp_switches.h")
README = os.path.join(ROOT, "tools", "README.md")
# listed in the table, read elsewhere: include/spp_adapter.h (header-only, built into applications) and the Python side
NOT_THE_LIBRARYS = {"SPP_ADAPTER_FLATTEN_THREADS", "SPP_LIB", "SPP_EXTRA_DEFS"}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _header_names():
    return re.findall(r'"(SPP_[A-Z0-9_]+)"', _read(HEADER))


def _readme_names():
    lines = _read(README).splitlines()
    start = lines.index("| switch | default | what it selects |")
    names = set()
    for line in lines[start + 2:]:
        if not line.startswith("|"):
            break
        names.update(re.findall(r"`(SPP_[A-Z0-9_]+)`", line.split("|")[1]))   # the row's first cell
    return names


def test_switch_header_matches_the_readme_table_and_alone_reads_the_environment():
    # (a) the same set of names on both sides, each parsed once
    header = _header_names()
    assert len(header) == len(set(header)), "a switch is parsed twice: %s" % sorted(n for n in header if header.count(n) > 1)
    readme = _readme_names()
    assert NOT_THE_LIBRARYS - {"SPP_EXTRA_DEFS"} <= readme   # (SPP_EXTRA_DEFS is described in the row of SPP_LIB)
    assert set(header) == readme - NOT_THE_LIBRARYS, (sorted(set(header) - readme), sorted(readme - NOT_THE_LIBRARYS - set(header)))
    # (b) no other file of the library reads the environment
    others = [f for f in sorted(os.listdir(CSRC)) if f != "spp_switches.h" and re.search(r"\bgetenv\b", _read(os.path.join(CSRC, f)))]
    assert others == [], others

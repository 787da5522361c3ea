"""CPU: the library's run-time switches are the documented few.  Every `getenv("VLQ_...")` under csrc/ names one of the
switches of DESIGN.md section 9, and every one of them is in that table -- an A/B switch does not grow back silently."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")

SWITCHES = {
    "VLQ_WALK_FIRST", "VLQ_WALK_SHARE", "VLQ_WALK_CLOCK", "VLQ_SCAN16_VARIANT", "VLQ_GENERIC_SCAN", "VLQ_IMI_MINSUM_LDS",
    "VLQ_SCAN_SCHEDULE", "VLQ_COARSE_FILTER", "VLQ_PHASE_TIMING", "VLQ_SCAN16_PHASES", "VLQ_L16C_TIMING",
}


def library_switches():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".cuh")):
            with open(os.path.join(CSRC, f)) as fh:
                names.update(re.findall(r'getenv\("(VLQ_[A-Z0-9_]+)', fh.read()))
    return names


def design_section_9():
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        text = fh.read()
    m = re.search(r"^## 9\..*?(?=^## |\Z)", text, re.M | re.S)
    assert m, "DESIGN.md has no section 9"
    return m.group(0)


def test_library_reads_only_the_documented_switches():
    assert library_switches() == SWITCHES


def test_every_switch_is_in_design_section_9():
    section = design_section_9()
    missing = sorted(n for n in SWITCHES if "`%s`" % n not in section)
    assert not missing, "not in DESIGN.md section 9: %s" % missing

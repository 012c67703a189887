"""No scratch memory in the fused pointwise backward: every k_pw<M_BDC, .., FTW > 0, ..> instance that the default FrostNet-Large @224 training step launches
(tests/golden/pw_fused_default_instances.txt, taken from a kernel trace of the replayed step) must compile for gfx950 without spilled vector registers and without a
private segment, at the kernel's own launch bound.  The test compiles csrc/frost_pw.hip to assembly with the project's flags and reads the two metadata fields
(.vgpr_spill_count, .private_segment_fixed_size) of each kernel; it needs no GPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LIST = os.path.join(ROOT, "tests", "golden", "pw_fused_default_instances.txt")


def instances():
    """Template arguments <MODE, WP, RES, FULLT, FTW, SP> of the listed instances, as tuples of ints."""
    out = []
    for line in open(LIST):
        line = line.split("#")[0].strip()
        if line:
            m = re.fullmatch(r"k_pw<(\d+), (\d+), (true|false), (true|false), (\d+), (\d+)>", line)
            assert m, line
            out.append(tuple(int(v) if v.isdigit() else int(v == "true") for v in m.groups()))
    return out


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the kernel metadata cannot be read")
    asm = str(tmp_path_factory.mktemp("pw_asm") / "frost_pw.s")
    subprocess.run([hipcc] + ge.FLAGS + ["--cuda-device-only", "-S", os.path.join(ge.CSRC, "frost_pw.hip"), "-o", asm], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    meta = {}
    for blk in open(asm).read().split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.fullmatch(r"_Z4k_pwILi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)ELi(\d+)EEv3PwP", name)
        if m:
            meta[tuple(int(v) for v in m.groups())] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in ("vgpr_spill_count", "private_segment_fixed_size"))
    return meta


def test_list_holds_fused_backward_instances():
    inst = instances()
    assert len(inst) >= 10 and len(set(inst)) == len(inst)
    assert all(i[0] == 3 and i[4] > 0 for i in inst), inst


def test_default_fused_backward_instances_use_no_scratch(metadata):
    bad = {}
    for i in instances():
        assert i in metadata, ("listed instance is not compiled", i)
        if metadata[i] != (0, 0):
            bad[i] = metadata[i]
    assert not bad, {k: dict(vgpr_spill_count=v[0], private_segment_fixed_size=v[1]) for k, v in bad.items()}

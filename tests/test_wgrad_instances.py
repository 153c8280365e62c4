"""CPU: the case table of the weight-gradient matrix (tests/wgrad_cases.py) reaches every kernel instance csrc/wgrad.hip
compiles to, and nothing else.  The unit is compiled device-only exactly as tools/spill_report.py does and the kernel names
of the resource-usage remarks are parsed: a new instance without a case, or a dispatch change that strands a case, fails
here on any machine.  Also the table's own conditions: every kernel family has an image of whole tiles, a ragged one and one
smaller than a tile, and every float64 reference stays small."""
import os
import re
import subprocess
import sys

import pytest

from wgrad_cases import (CASES, REF_MADD_CAP, SPLIT_CASES, Case, family_of, image_kind, instance_of, ref_madds, tile_rows,
                         tiles_of, workgroup_shape)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image_segmentation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def parse_instance(mangled):
    """Mangled kernel name -> the spelling instance_of() uses, or None for anything that is not a wgrad kernel."""
    m = re.search(r"16wgrad_dma_kernelILi(\d)ELi(\d)ELb([01])ELb([01])EE", mangled)
    if m:
        b = lambda v: "true" if v == "1" else "false"
        return f"wgrad_dma_kernel<{m.group(1)},{m.group(2)},{b(m.group(3))},{b(m.group(4))}>"
    m = re.search(r"12wgrad_kernelI(DF16b|f)Li(\d)ELi(\d)ELi(\d)EE", mangled)      # DF16b: __bf16 (c++filt garbles it)
    if m:
        return f"wgrad_kernel<{'bf16' if m.group(1) == 'DF16b' else 'fp32'},{m.group(2)},{m.group(3)},{m.group(4)}>"
    return None


@pytest.fixture(scope="module")
def compiled_instances():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import spill_report
    finally:
        sys.path.pop(0)
    rows = spill_report.report("wgrad")
    assert rows, "the resource-usage remarks of wgrad.hip were not found"
    names = [parse_instance(r["name"]) for r in rows]
    assert None not in names, [r["name"] for r, n in zip(rows, names) if n is None]
    assert len(set(names)) == len(names)
    return set(names)


def test_parse_instance():
    assert parse_instance("_ZN12_GLOBAL__N_116wgrad_dma_kernelILi4ELi2ELb1ELb0EEEv9WgradArgs") == "wgrad_dma_kernel<4,2,true,false>"
    assert parse_instance("_ZN12_GLOBAL__N_112wgrad_kernelIDF16bLi2ELi4ELi2EEEv9WgradArgs") == "wgrad_kernel<bf16,2,4,2>"
    assert parse_instance("_ZN12_GLOBAL__N_112wgrad_kernelIfLi1ELi1ELi2EEEv9WgradArgs") == "wgrad_kernel<fp32,1,1,2>"
    assert parse_instance("_ZN12_GLOBAL__N_119wgrad_reduce_kernelEPKfiPfiiiiiii") is None


@pytest.mark.timeout(600)
def test_table_reaches_every_compiled_instance(compiled_instances):
    table = {instance_of(c) for c in CASES}
    missing, stranded = compiled_instances - table, table - compiled_instances
    print(f"{len(compiled_instances & table)} of {len(compiled_instances)} compiled instances matched by the table")
    assert not missing, f"compiled instances without a case: {sorted(missing)}"
    assert not stranded, f"cases whose instance is not compiled (dispatch changed?): {sorted(stranded)}"
    assert len(compiled_instances) == 45


def test_instance_of_follows_the_dispatch_rules():
    mk = lambda **k: Case(**{**dict(geo=0, dtype="bf16", CD=64, CA=64, CB=0, B=1, H=16, W=32, prologue=False, zero_page=True), **k})
    assert instance_of(mk()) == "wgrad_dma_kernel<2,2,false,false>"
    assert instance_of(mk(CD=128, prologue=True)) == "wgrad_dma_kernel<4,2,true,false>"       # the benchmark's instance
    assert instance_of(mk(CD=128, CA=96)) == "wgrad_dma_kernel<2,1,false,false>"              # 4 x 2 needs CA % 64 == 0
    assert instance_of(mk(CD=128, CB=32)) == "wgrad_dma_kernel<2,1,false,false>"              # ... and CB % 64 == 0
    assert instance_of(mk(H=14)) == "wgrad_dma_kernel<2,2,false,true>"
    assert instance_of(mk(W=17)) == "wgrad_dma_kernel<2,2,false,true>"
    assert instance_of(mk(CD=128, zero_page=False)) == "wgrad_kernel<bf16,0,2,2>"
    assert instance_of(mk(CD=128, dtype="fp32")) == "wgrad_kernel<fp32,0,2,2>"
    assert instance_of(mk(CD=128, geo=1)) == "wgrad_kernel<bf16,1,2,2>"
    assert instance_of(mk(CD=128, geo=2)) == "wgrad_kernel<bf16,2,4,2>" and tile_rows(mk(CD=128, geo=2)) == 8
    assert instance_of(mk(CD=96, CA=32, geo=2, dtype="fp32")) == "wgrad_kernel<fp32,2,1,1>"
    assert tile_rows(mk(geo=2)) == 4 and tile_rows(mk(geo=2, dtype="fp32")) == 2 and tile_rows(mk(dtype="fp32")) == 4


def test_every_instance_has_whole_and_ragged_images_and_every_family_a_sub_tile_one():
    kinds = {}
    for c in CASES:
        kinds.setdefault(family_of(c), set()).add(image_kind(c))
    assert len(kinds) == 8, sorted(kinds)
    for fam, k in kinds.items():
        assert {"whole", "ragged", "sub-tile"} <= k, (fam, k)
    # the LDS-DMA instances split on whole / not whole tiles; every other instance must see both kinds of image itself
    per = {}
    for c in CASES:
        per.setdefault(instance_of(c), set()).add(image_kind(c))
    for name, k in per.items():
        if name.startswith("wgrad_dma_kernel"):
            assert k == ({"ragged", "sub-tile"} if name.endswith("true>") else {"whole"}), (name, k)
        else:
            assert {"whole", "ragged", "sub-tile"} <= k, (name, k)


def test_table_conditions():
    assert len(set(CASES)) == len(CASES)
    for c in CASES + SPLIT_CASES:
        assert c.CD % 32 == 0 and c.CA % 32 == 0 and c.CB % 32 == 0 and c.CA > 0
        assert not (c.prologue and c.CB), "the prologue form has one source"
        assert ref_madds(c) <= REF_MADD_CAP, c
    concat = [c for c in CASES if c.CB]
    assert all(c.CA != c.CB for c in concat)
    assert any(c.CA % 64 == 0 and c.CB % 64 != 0 and workgroup_shape(c)[1] == 1 for c in concat)
    assert any(workgroup_shape(c)[1] == 2 for c in concat)
    # channel counts reaching each shape at two widths
    assert {c.CD for c in CASES} >= {32, 96, 64, 192, 128, 256} and {c.CA for c in CASES} >= {32, 96, 64, 128}
    # prologue on every LDS-DMA shape, on whole-tile and ragged images
    pro = {instance_of(c) for c in CASES if c.prologue and c.zero_page and c.dtype == "bf16"}
    assert len(pro) == 10
    fams = {family_of(c) if c.geo != 2 else instance_of(c) for c in SPLIT_CASES}
    assert fams == {"dma", "dma+prologue", "staged-fp32-geo0", "staged-bf16-geo1", "wgrad_kernel<bf16,2,2,2>",
                    "wgrad_kernel<bf16,2,4,2>"}
    assert all(tiles_of(c) >= 4 for c in SPLIT_CASES)

"""CPU: the case table of the 1x1-geometry matrix (tests/gemm_cases.py) reaches every instance of gemm_dma_kernel
(csrc/gemm.hip), of convt_stream_kernel (csrc/convt_stream.hip) and every GEO == 1 instance of conv_igemm_kernel
(csrc/conv_igemm.hip) the units compile to, without exception, and nothing else.  The units
are compiled device-only exactly as tools/spill_report.py does and the kernel names of the resource-usage remarks are parsed
(names and register counts only): a new instance without a case, or a dispatch change that strands a case, fails here on any
machine.  Also the table's own conditions: image kinds per instance, the W = 16 / 17 pairs, the pixel-shuffle cases whose tap
boundary falls inside a column tile, every wave layout of the streaming kernel, both row tiles of the LDS-DMA GEMM in every
mode, and the cases with three or more work units (blocks) per workgroup (stream).  The launch arithmetic is evaluated for
256 compute units; tests/test_gpu_gemm_matrix.py asserts that the device has as many."""
import itertools
import os
import re
import sys

import pytest

from gemm_cases import (CASES, LONG_CASES, NUM_CUS, PERSISTENT_FAMILIES, blocks_per_stream, case_id, convt_stream_ok,
                        dma_bm, family_of, gemm_dma_ok, gemm_view, image_kind, instance_of, is_valid, kernel_of, lin, min_chunks, mk,
                        nchunks_of, rows_of, select, spell, splitk_ok, stream_grid, tile_shape, unit_walk, units_per_workgroup)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def parse_instance(mangled):
    """Mangled kernel name -> the spelling kernel_of() uses; None for a 3x3 (GEO == 0) instance of conv_igemm_kernel, which
    tests/test_conv_instances.py accounts for, and for every other kernel."""
    m = re.search(r"15gemm_dma_kernelILi(\d)ELi(\d+)EE", mangled)
    if m:
        return f"gemm_dma_kernel<{m.group(1)},{m.group(2)}>"
    m = re.search(r"19convt_stream_kernelILi(\d)ELi(\d)ELi(\d)EE", mangled)
    if m:
        return f"convt_stream_kernel<{m.group(1)},{m.group(2)},{m.group(3)}>"
    m = re.search(r"17conv_igemm_kernelI(DF16b|f)Li(\d)E" + r"Li(\d)E" * 6 + r"Lb([01])EE", mangled)
    if m and m.group(2) == "1":
        return "conv_igemm_kernel<{},1,{},{},{},{},{},{},{}>".format("bf16" if m.group(1) == "DF16b" else "fp32", *m.group(3, 4, 5, 6, 7, 8),
                                                                     "true" if m.group(9) == "1" else "false")
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
    names = []
    for unit, kernel in (("gemm", "gemm_dma_kernel"), ("convt_stream", "convt_stream_kernel"), ("conv_igemm", "conv_igemm_kernel")):
        rows = spill_report.report(unit)
        assert rows, f"the resource-usage remarks of {unit}.hip were not found"
        mine = [parse_instance(r["name"]) for r in rows if kernel in r["name"]]
        if unit != "conv_igemm":          # every kernel of these two units belongs to the matrix
            assert len(mine) == len(rows) and None not in mine, [r["name"] for r in rows]
        names += [n for n in mine if n is not None]
    assert len(set(names)) == len(names)
    return set(names)


def test_parse_instance():
    p = parse_instance
    assert p("_ZN12_GLOBAL__N_115gemm_dma_kernelILi1ELi320EEEv8GemmArgs") == "gemm_dma_kernel<1,320>"
    assert p("_ZN12_GLOBAL__N_119convt_stream_kernelILi8ELi4ELi1EEEvPKDF16bS2_PKfPS0_iiiii") == "convt_stream_kernel<8,4,1>"
    assert p("_ZN12_GLOBAL__N_117conv_igemm_kernelIfLi1ELi5ELi8ELi1ELi1ELi1ELi2ELb0EEEv8ConvArgs") == \
        "conv_igemm_kernel<fp32,1,5,8,1,1,1,2,false>"
    assert p("_ZN12_GLOBAL__N_117conv_igemm_kernelIDF16bLi1ELi4ELi2ELi2ELi2ELi1ELi2ELb0EEEv8ConvArgs") == \
        "conv_igemm_kernel<bf16,1,4,2,2,2,1,2,false>"
    assert p("_ZN12_GLOBAL__N_117conv_igemm_kernelIDF16bLi0ELi4ELi2ELi2ELi2ELi1ELi1ELb1EEEv8ConvArgs") is None      # GEO == 0
    assert p("_ZN12_GLOBAL__N_114conv_ws_kernelIDF16bLi5ELb1EEEv8ConvArgs") is None


@pytest.mark.timeout(900)
def test_table_accounts_for_every_compiled_instance(compiled_instances):
    table = {kernel_of(c) for c in CASES}
    print(f"{len(compiled_instances & table)} of {len(compiled_instances)} compiled 1x1-geometry instances reached by the table")
    missing, stranded = compiled_instances - table, table - compiled_instances
    assert not missing, f"compiled instances without a case: {sorted(missing)}"
    assert not stranded, f"cases whose instance is not compiled (dispatch changed?): {sorted(stranded)}"
    assert len(compiled_instances) == 19          # 6 gemm_dma + 3 convt_stream + 10 conv_igemm<*, 1, ...>
    assert {kernel_of(c) for c in LONG_CASES} <= table


def test_every_case_is_a_valid_call_and_distinct():
    assert len(set(CASES)) == len(CASES) and not set(CASES) & set(LONG_CASES)
    for c in CASES + LONG_CASES:
        assert is_valid(c), c
    assert len({case_id(c) for c in CASES + LONG_CASES}) == len(CASES) + len(LONG_CASES)
    assert len(CASES) <= 200
    # logical channel counts below the padding: 40 of 64 in and 70 of 96 out among them, on ragged images
    short = [c for c in CASES if (c.Lin, c.Lout) != (c.Cin, c.Cout)]
    assert {c.entry for c in short} == {"linear", "conv1x1", "convt_fwd", "convt_dgrad"}
    assert any((c.Lin, c.Cin, c.Lout, c.Cout) == (40, 64, 70, 96) for c in short)
    assert all(image_kind(c) in ("ragged", "whole") for c in short) and sum(image_kind(c) == "ragged" for c in short) >= 10
    assert {family_of(c).rsplit("-", 1)[0] if family_of(c).startswith("dma") else family_of(c) for c in short} == \
        {"dma-0", "dma-1", "dma-2", "generic-bf16", "generic-fp32", "stream-0", "stream-1"}


def _sweep():
    """every instance the mirror selects over the padded channel counts, widths, row counts and entries"""
    seen = set()
    chans = list(range(32, 321, 32)) + [512, 576, 1024, 2560]
    imgs = [(1, 1, 1), (1, 1, 16), (2, 8, 16), (2, 8, 17), (2, 16, 64), (2, 8, 197), (2, 8, 200), (16, 19, 19)]
    for dtype, (B, H, W), cin, cout in itertools.product(("bf16", "fp32"), imgs, chans, chans):
        for entry in ("conv1x1", "convt_fwd", "convt_dgrad"):
            seen.add(kernel_of(mk(entry, dtype, B, H, W, cin, cout)))
    for dtype, M, K, N in itertools.product(("bf16", "fp32"), (16, 128, 272, 3152, 3200, 6160), chans, chans):
        seen.add(kernel_of(lin(dtype, M, K, N, 0)))
        for S in (1, 2, 3, 4):
            c = lin(dtype, M, K, N, S)
            if is_valid(c):
                seen.add(kernel_of(c))
    return seen


def test_sweep_of_the_mirror_selects_exactly_the_tables_instances():
    assert _sweep() == {kernel_of(c) for c in CASES}


def test_instance_of_follows_the_dispatch_rules():
    """shapes of the real models (256 compute units)"""
    assert NUM_CUS == 256
    # CLIP ViT-B/16 at B = 16: 3152 token rows.  fc1 is the shape the 320-row tile was written for: 240 units, one round
    assert instance_of(lin("bf16", 3152, 768, 3072, 0, True, 1)) == "gemm_dma_kernel<0,320>"
    assert units_per_workgroup(lin("bf16", 3152, 768, 3072, 0, True, 1)) == 1
    assert instance_of(lin("bf16", 3152, 768, 2304, 0, True)) == "gemm_dma_kernel<0,256>"          # qkv: 234 units
    assert instance_of(lin("bf16", 3152, 3072, 768, 3, True)) == "gemm_dma_kernel<0,256>"          # fc2, split three ways: 234
    assert instance_of(lin("bf16", 3152, 768, 768, 3, True)) == "gemm_dma_kernel<0,256>"           # out projection
    assert instance_of(lin("fp32", 3152, 768, 3072, 0, True, 1)) == "conv_igemm_kernel<fp32,1,4,4,2,2,2,2,false>"
    assert instance_of(lin("bf16", 3152, 96, 64, 0, True, 1)) == "conv_igemm_kernel<bf16,1,4,2,2,2,1,2,false>"
    # U-Net up1 .. up4 at B = 32 on a 256 x 256 image: 1024 -> 512 at 16 x 16 ... 128 -> 64 at 128 x 128
    up = [mk("convt_fwd", "bf16", 32, 16 << i, 16 << i, 1024 >> i, 512 >> i, bias=True) for i in range(4)]
    assert [instance_of(c) for c in up] == ["gemm_dma_kernel<1,256>", "gemm_dma_kernel<1,256>", "convt_stream_kernel<8,4,0> wpc=8",
                                            "convt_stream_kernel<4,8,0> wpc=2"]
    dg = [instance_of(c._replace(entry="convt_dgrad", bias=False)) for c in up]
    assert dg == ["gemm_dma_kernel<2,256>", "gemm_dma_kernel<2,256>", "gemm_dma_kernel<2,256>", "convt_stream_kernel<8,4,1> wpc=2"]
    assert all(units_per_workgroup(c) >= 2 for c in up[:2]) and blocks_per_stream(up[3]) >= 3      # the real layers cross unit boundaries
    # the CLIP decoder's 1x1 convolutions on the 14 x 14 token grid (B = 16): 768 -> 512 | 256 | 128 | 64
    clip = [instance_of(mk("conv1x1", "bf16", 16, 14, 14, 768, n, bias=True)) for n in (512, 256, 128, 64)]
    assert clip == ["gemm_dma_kernel<0,256>"] * 3 + ["conv_igemm_kernel<bf16,1,4,2,2,2,1,2,false>"]
    assert instance_of(mk("conv1x1", "fp32", 16, 14, 14, 768, 64, bias=True)) == "conv_igemm_kernel<fp32,1,4,4,2,2,1,2,false>"
    assert instance_of(mk("conv1x1", "fp32", 16, 28, 28, 768, 96)) == "conv_igemm_kernel<fp32,1,5,8,1,1,1,2,false>"
    # the predicates themselves
    assert min_chunks(1) == 16 and min_chunks(0) == min_chunks(2) == 8
    assert gemm_dma_ok(128, 8, 8, 128, 128, 256, 0) and not gemm_dma_ok(112, 8, 8, 128, 128, 256, 0)
    assert not gemm_dma_ok(128, 9, 9, 128, 128, 288, 0) and not gemm_dma_ok(128, 8, 8, 192, 192, 256, 0)
    assert gemm_dma_ok(128, 8, 2, 128, 128, 64, 2) and not gemm_dma_ok(128, 12, 3, 128, 128, 96, 2)
    assert not gemm_dma_ok(128, 14, 14, 128, 32, 448, 1) and gemm_dma_ok(128, 16, 16, 128, 32, 512, 1)
    assert not gemm_dma_ok(1 << 22, 16, 16, 128, 128, 512, 0) and gemm_dma_ok((1 << 22) - 16, 16, 16, 128, 128, 512, 0)
    assert convt_stream_ok(1, 1, 16, 128, 256, "bf16") and not convt_stream_ok(1, 1, 16, 128, 96, "bf16")
    assert not convt_stream_ok(1, 1, 16, 256, 256, "bf16") and not convt_stream_ok(1, 1, 17, 128, 64, "bf16")
    assert not convt_stream_ok(1, 1, 16, 128, 64, "fp32")
    assert splitk_ok(128, 256, 128, 4) and not splitk_ok(128, 192, 128, 3) and not splitk_ok(3152, 768, 768, 5)
    assert dma_bm(3152, 3072, 1) == 320 and dma_bm(3152, 2304, 1) == 256 and dma_bm(3152, 768, 3) == 256


def test_every_instance_has_its_image_kinds():
    per = {}
    for c in CASES:
        per.setdefault(instance_of(c), set()).add(image_kind(c))
        if image_kind(c) == "ragged" and select(c)[0] == "generic" and c.entry != "linear":
            assert c.B >= 2, c
    assert len(per) == 24          # 6 + 10 + the 8 wave layouts of the three streaming instances
    for name, kinds in per.items():
        if name.startswith("gemm_dma_kernel") and name.endswith(",256>"):
            assert {"min", "whole", "tile+16", "ragged"} <= kinds, (name, kinds)      # M = 128, M = BM, M = BM + 16
        elif name.startswith("gemm_dma_kernel"):          # 320-row tiles are taken for large problems only
            assert {"whole", "ragged"} <= kinds, (name, kinds)
        elif name.startswith("convt_stream"):
            assert {"whole", "sub-tile"} <= kinds, (name, kinds)
        else:
            assert {"whole", "ragged", "sub-tile"} <= kinds, (name, kinds)
    # the sub-tile problems: M = 16 for segk_linear, a 1 x 1 image for the convolution entries, 1 x 16 for the streaming kernel
    for c in CASES:
        if image_kind(c) == "sub-tile" and select(c)[0] == "generic":
            assert rows_of(c) == 16 if c.entry == "linear" else (c.H, c.W) in ((1, 1), (3, 17)), c
    for fam in ("generic-bf16", "generic-fp32"):
        for e in ("conv1x1", "convt_fwd", "convt_dgrad"):
            assert any(family_of(c) == fam and c.entry == e and (c.B, c.H, c.W) == (1, 1, 1) for c in CASES), (fam, e)
        assert any(family_of(c) == fam and c.entry == "linear" and rows_of(c) == 16 for c in CASES), fam
    # segk_linear reaches the generic kernel at W = 16 only; every other generic instance is reached by a convolution entry
    for name in per:
        if name.startswith("conv_igemm"):
            assert any(instance_of(c) == name and c.entry != "linear" for c in CASES), name


def test_w16_and_w17_pairs_wherever_the_instance_depends_on_the_width():
    table = set(CASES)
    pairs = set()
    for c in CASES:
        if c.W == 16 and c._replace(W=17) in table and instance_of(c) != instance_of(c._replace(W=17)):
            pairs.add((instance_of(c), instance_of(c._replace(W=17))))
    wdep = {instance_of(c) for c in CASES if select(c)[0] == "generic" and
            instance_of(c._replace(W=16)) != instance_of(c._replace(W=17)) and c.entry != "linear"}
    assert wdep == {i for ab in pairs for i in ab}, sorted(wdep ^ {i for ab in pairs for i in ab})
    assert len(wdep) == 8          # bf16: the N % 32 form; fp32: all three


def test_pixel_shuffle_cases_put_the_tap_boundary_inside_a_column_tile():
    fwd = {}
    for c in CASES:
        if c.entry == "convt_fwd":
            fwd.setdefault(instance_of(c), set()).add(c.Cout)
    for name, couts in fwd.items():
        if name.startswith("convt_stream"):
            continue
        if name.endswith(",320>"):          # large problems only: Cout = 640, five column tiles per tap
            assert couts == {640}
            continue
        assert {32, 96, 160} <= couts, (name, couts)
    assert set(fwd) >= {"gemm_dma_kernel<1,256>", "gemm_dma_kernel<1,320>", "conv_igemm_kernel<bf16,1,4,2,2,2,2,2,false>",
                        "conv_igemm_kernel<fp32,1,4,4,2,2,2,2,false>", "conv_igemm_kernel<fp32,1,5,4,2,2,2,2,false>"}
    # every wave layout of the two streaming forward instances, and the one of the data gradient
    wpc = {instance_of(c) for c in CASES if select(c)[0] == "stream"}
    assert wpc == {f"convt_stream_kernel<4,8,0> wpc={w}" for w in (1, 2, 4, 8)} | {f"convt_stream_kernel<8,4,0> wpc={w}" for w in (2, 4, 8)} \
        | {"convt_stream_kernel<8,4,1> wpc=2"}
    assert {c.Cout for c in CASES if kernel_of(c) == "convt_stream_kernel<4,8,0>"} == {32, 64, 128, 256}
    assert {c.Cout for c in CASES if kernel_of(c) == "convt_stream_kernel<8,4,0>"} == {32, 64, 128}
    # the un-shuffle gather of the LDS-DMA GEMM: two chunks per tap (the least) and larger even counts
    ncha = {c.Cout // 32 for c in CASES if family_of(c).startswith("dma-2")}
    assert 2 in ncha and len(ncha) >= 3 and all(n % 2 == 0 for n in ncha)


def test_k_counts_bias_activation_and_split():
    dma = {}
    for c in CASES:
        if select(c)[0] == "dma":
            dma.setdefault(select(c)[1][0], []).append(c)
    for mode, cs in dma.items():
        n = {nchunks_of(c) // c.S for c in cs}          # chunks per unit
        assert min(nchunks_of(c) for c in cs) == min_chunks(mode), mode
        assert any(k % 5 and k % 6 for k in n) and any(k > 12 for k in n), (mode, n)
        assert {256, 320} == {select(c)[1][1] for c in cs}, mode
    assert {10, 14} <= {nchunks_of(c) for c in dma[0]} and 26 in {nchunks_of(c) for c in dma[0]}
    split = [c for c in CASES if c.entry == "linear_splitk"]
    assert {c.S for c in split} >= {1, 2, 3} and any(nchunks_of(c) // c.S == 2 for c in split)
    assert {select(c)[1][1] for c in split if c.S > 1} == {256, 320} and {c.bias for c in split} == {False, True}
    by = {}
    for c in CASES:
        by.setdefault(kernel_of(c), []).append(c)
    for name, cs in by.items():
        if name != "convt_stream_kernel<8,4,1>" and not name.startswith("gemm_dma_kernel<2"):      # the data gradient has no bias
            assert {c.bias for c in cs} == {False, True}, name
        plain = [c for c in cs if c.entry == "linear"]
        if plain:          # quick_gelu on every instance segk_linear reaches
            assert any(c.act for c in plain), name
    assert {kernel_of(c) for c in CASES if c.act} == {kernel_of(c) for c in CASES if c.entry == "linear"}
    assert any(c.act and c.dtype == "fp32" and nchunks_of(c) >= 16 for c in CASES)


def test_three_or_more_units_per_workgroup_in_every_persistent_family():
    assert {family_of(c) for c in LONG_CASES} == set(PERSISTENT_FAMILIES) == {family_of(c) for c in CASES}
    for c in LONG_CASES:
        form, p = select(c)
        if form == "stream":
            nblk, g, streams = stream_grid(c)
            trips = blocks_per_stream(c)
            assert trips >= 3 and trips % 2 == 1 and nblk % (g * streams) != 0 and g == NUM_CUS, c
        else:
            assert units_per_workgroup(c) >= 3, c
        if form == "dma":          # consecutive units of a workgroup change row tile, column tile and (split-K) the K range
            w = unit_walk(c)
            assert len(w) == units_per_workgroup(c)
            for i in range(3 if c.S > 1 else 2):
                assert any(a[i] != b[i] for a, b in zip(w, w[1:])), (c, w)
            assert (nchunks_of(c) // c.S) % (6 if p[1] == 256 else 5), c          # a unit ends inside the ring (six | five slots)
    assert sum(c.S > 1 for c in LONG_CASES) == 2 and {select(c)[1][1] for c in LONG_CASES if c.S > 1} == {256, 320}
    # the smallest and the largest wave layout of each streaming forward instance
    assert {instance_of(c) for c in LONG_CASES if select(c)[0] == "stream"} == {
        "convt_stream_kernel<4,8,0> wpc=1", "convt_stream_kernel<4,8,0> wpc=8", "convt_stream_kernel<8,4,0> wpc=2",
        "convt_stream_kernel<8,4,0> wpc=8", "convt_stream_kernel<8,4,1> wpc=2"}
    # the three-run cases stay small: one unit per workgroup, one block per stream
    for c in CASES:
        assert (blocks_per_stream(c) if select(c)[0] == "stream" else units_per_workgroup(c)) == 1, c
    for c in CASES + LONG_CASES:          # every buffer under about 100 MB
        M, K, N, _ = gemm_view(c)
        assert max(M * K, M * N * c.S) * (2 if c.dtype == "bf16" else 4) <= 100 * 10 ** 6, c

"""CPU: the measurement tooling parses before any GPU minute is spent on it -- every tools/*.py compiles, every tools/*.sh
passes `bash -n`, and no shell script embeds Python in a heredoc (round-2 finding: a quoting error inside such a heredoc let
five rocprofv3 passes run and then died before writing their summary)."""
import glob
import os
import py_compile
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tool_scripts_parse():
    pys = sorted(glob.glob(os.path.join(ROOT, "tools", "*.py")))
    assert pys
    for p in pys:
        py_compile.compile(p, doraise=True)
    shs = sorted(glob.glob(os.path.join(ROOT, "tools", "*.sh")))
    assert shs
    for p in shs:
        r = subprocess.run(["bash", "-n", p], capture_output=True, text=True)
        assert r.returncode == 0, (p, r.stderr)
        assert not re.search(r"python3?\s+-\s*<<", open(p).read()), f"{p}: Python heredoc -- move it into tools/pmc_post.py"


def test_pmc_post_names_kernel_families():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pmc_post", os.path.join(ROOT, "tools", "pmc_post.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    n = "void (anonymous namespace)::conv3x3_pipe_kernel<5, false, 128, true>(ConvArgs)"
    assert m.short(n) == "conv3x3_pipe_kernel<5, false, 128, true>" and m.family(n) == "conv3x3"
    assert m.family("void (anonymous namespace)::wgrad_dma_kernel<4, 2, false>(WgradArgs)") == "wgrad3x3"
    assert m.family("_ZN12_GLOBAL__N_112wgrad_kernelIDF16bLi2ELi4ELi2EEEv9WgradArgs") == "wgrad_other"
    assert m.family("void at::native::vectorized_elementwise_kernel<4>(int)") is None


def test_no_undefined_names_in_product_python():
    """A static pass over the package and bench.py: every name that is read is bound somewhere in its module (assignment,
    def, class, import, argument, loop / comprehension / with / except target) or is a builtin.  Catches a helper deleted by
    an edit (a NameError that only a GPU run would otherwise show)."""
    import ast
    import builtins
    files = sorted(glob.glob(os.path.join(ROOT, "image_segmentation_amd", "*.py"))) + [os.path.join(ROOT, "bench.py"),
                                                                                       os.path.join(ROOT, "__graft_entry__.py")]
    for path in files:
        tree = ast.parse(open(path).read(), path)
        bound = set(dir(builtins)) | {"__file__", "__name__", "__doc__"}
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                bound.add(node.name)
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                a = node.args
                for arg in a.posonlyargs + a.args + a.kwonlyargs + ([a.vararg] if a.vararg else []) + ([a.kwarg] if a.kwarg else []):
                    bound.add(arg.arg)
            elif isinstance(node, ast.Name) and isinstance(node.ctx, (ast.Store, ast.Del)):
                bound.add(node.id)
            elif isinstance(node, (ast.Import, ast.ImportFrom)):
                for al in node.names:
                    bound.add((al.asname or al.name).split(".")[0])
            elif isinstance(node, ast.ExceptHandler) and node.name:
                bound.add(node.name)
            elif isinstance(node, (ast.Global, ast.Nonlocal)):
                bound.update(node.names)
        missing = sorted({n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load)} - bound)
        assert not missing, (os.path.relpath(path, ROOT), missing)


def _load_tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_streaming_and_finalize_kernels_keep_their_loads_in_flight():
    """Compiled-code check (hipcc cross-compiles here): the HBM-bound helper kernels must not contain loads that wait for
    themselves, and must not spill.  Round-3 finding: `cond ? p[i] : 0` compiles to branch + load + s_waitcnt vmcnt(0), which
    turned every "N rows in flight" finalize walk of the library into N serial memory round trips (loss finalize 32 us,
    BatchNorm finalize kernels 8-9 us each, 36 per step), and a fully unrolled LDS sum spilled 16 registers."""
    ser = _load_tool("serialized_loads")
    hot = ("bn_bwd_finalize_kernel", "bn_stats_finalize_small_kernel", "maxpool_bwd_kernel", "bn_relu_apply_pool_kernel",
           "bn_bwd_reduce_kernel", "loss_fwd_kernel", "loss_bwd_kernel", "head_fwd_kernel", "wgrad_reduce_kernel",
           "wgrad_reduce_wide_kernel")       # (stem_wgrad keeps conditional loads on its image-border path: measured faster)
    seen = set()
    for unit in ("bn_pool", "head", "loss", "pack", "stem"):
        for n_ser, n_loads, _, name in ser.scan(unit):
            for h in hot:
                if h in name or h[:-7] in name:        # (mangled names of template kernels carry the stem only)
                    seen.add(h)
                    assert n_ser <= 2, f"{name}: {n_ser} of {n_loads} loads wait for themselves"
    assert len(seen) >= 9, seen
    rep = _load_tool("spill_report")
    for unit in ("bn_pool", "head", "loss", "pack", "stem"):
        for r in rep.report(unit):
            assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, (unit, r)


def test_no_inline_asm_arithmetic_on_vector_registers():
    """Inline-asm VALU instructions are invisible to the compiler's hazard recogniser: placed right behind an MFMA they read
    the accumulator before the matrix pipe has written it (round 3: `v_cvt_pk_bf16_f32` as asm in the ConvTranspose streaming
    kernel returned garbage once the index arithmetic between MFMA and conversion got shorter).  Conversions go through
    `cvt_pk_bf16()` (a vector conversion the compiler lowers to the same instruction, with the wait states); the only VALU
    asm allowed is the lane-id idiom."""
    bad = []
    for path in sorted(glob.glob(os.path.join(ROOT, "image_segmentation_amd", "csrc", "*.h*"))):
        for ln, line in enumerate(open(path), 1):
            code = line.split("//")[0]
            m = re.search(r'asm[^"]*"\s*(v_\w+)', code)
            if m and not m.group(1).startswith("v_mbcnt"):
                bad.append((os.path.basename(path), ln, m.group(1)))
    assert not bad, bad

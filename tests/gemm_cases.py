"""GEMM test cases as text, shared by the GPU and the CPU tests.

A *signature* ``MxNxK:<a><b>:<out>:<act><act_bwd>:<flags>`` is a key of ``ops/gemm_tuned.json``
(layouts k / m, output f / h, activation codes, flags b bias, x aux_out, r residual, c column
sums, a accumulate).  A *case* is a signature followed by ``key=value`` settings, as
``tests/tools/gemm_plan_tool.cpp`` reads them and ``tests/golden/gemm_plan_cases.txt`` records
them with the dispatcher's plan.

The CPU half (this file imports no torch at module level): which recorded case exercises which
compiled instantiation of the persistent family, and how such a case is grown until one
workgroup streams two units.  The GPU half: operands for a signature, and running a case with
its settings applied and the plan checked.
"""
from __future__ import annotations

import contextlib
import os
import re
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = os.path.join(ROOT, "distributed_pytorch_cookbook_amd", "ops")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_cases.txt")
KERNEL_RE = re.compile(r"gemm(?:7|7d|9)_kernel<[^>]*>")

# settings of a case that a running process can apply: GemmArgs fields (impl, ws, deriv) and the
# library's setters.  Not nt= (read from the environment once), not xcd= (it does not touch the
# persistent family) and not the requirement-failure keys (coff ldc ac bc ldi ldo).
RUNTIME_KEYS = frozenset(("impl", "ws", "deriv", "gimpl", "splits", "reserve", "actlds", "reslds"))
# a reserve beyond the CU count leaves the smallest grid: 8 workgroups (16 slots for v8)
SMALL_GRID = 1000
MAX_GROW = 20  # tiles added along M and N in the search for a two-unit case (v8: 17 units on one short side)


def parse_sig(sig: str):
    dims, lay, out, acts, flags = sig.split(":")
    M, N, K = (int(x) for x in dims.split("x"))
    return M, N, K, lay[0] == "k", lay[1] == "k", out == "f", int(acts[0]), int(acts[1]), flags


def parse_case(case: str):
    """-> (signature, {key: int})"""
    sig, *toks = case.split()
    return sig, {k: int(v) for k, v in (t.split("=") for t in toks)}


def format_case(sig: str, st: dict) -> str:
    return " ".join([sig] + [f"{k}={v}" for k, v in st.items()])


def identities() -> list:
    """The compiled instantiations of the persistent family (ops/csrc/gemm_parts.txt), in file order."""
    with open(os.path.join(OPS, "csrc", "gemm_parts.txt")) as f:
        return [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]


def golden() -> list:
    """[(case, plan text)] of the recorded dispatcher answers."""
    with open(GOLDEN) as f:
        return [tuple(ln.rstrip("\n").split("\t")) for ln in f if ln.strip()]


def runnable(case: str) -> bool:
    sig, st = parse_case(case)
    act, flags = parse_sig(sig)[6], parse_sig(sig)[8]
    if not set(st) <= RUNTIME_KEYS:
        return False
    return not st.get("deriv") or (act == 2 and "x" in flags)  # (ops/gemm.py refuses aux_deriv otherwise)


def volume(case: str) -> int:
    M, N, K = parse_sig(parse_case(case)[0])[:3]
    return M * N * K


def cases_by_identity() -> dict:
    """identity -> the recorded cases that name it and can be set up at run time, smallest volume
    first (ties: in the golden file's order)."""
    by = {}
    for case, plan in golden():
        if runnable(case):
            for ident in set(KERNEL_RE.findall(plan)):
                by.setdefault(ident, []).append(case)
    return {ident: sorted(dict.fromkeys(cs), key=volume) for ident, cs in by.items()}


def smallest_cases() -> dict:
    """identity -> its smallest runnable recorded case"""
    return {ident: cs[0] for ident, cs in cases_by_identity().items()}


def g7_fields(plan: str):
    """(tiles_m, tiles_n, tile_n, units, grid, nk, nk_all, splits, store_cnt, debug) of a plan, or None"""
    m = re.search(r" g7=([\d,]+)", plan)
    return tuple(int(v) for v in m.group(1).split(",")) if m else None


def streams_two_units(ident: str, plan: str) -> bool:
    g7 = g7_fields(plan)
    return ident in plan and g7 is not None and g7[3] > g7[4]


def grown_candidates(case: str, tile_n: int) -> list:
    """``case`` on the smallest grid, grown by tm tiles along M and tn along N, tm + tn <=
    MAX_GROW, the smallest output first."""
    sig, st = parse_case(case)
    dims, rest = sig.split(":", 1)
    M, N, K = (int(v) for v in dims.split("x"))
    st = dict(st, reserve=SMALL_GRID)
    grown = sorted(((M + 256 * tm) * (N + tile_n * tn), tm, tn) for tm in range(MAX_GROW + 1)
                   for tn in range(MAX_GROW + 1 - tm))
    return [format_case(f"{M + 256 * tm}x{N + tile_n * tn}x{K}:{rest}", st) for _, tm, tn in grown]


def two_unit_case(ident: str, bases: list, explain):
    """The first grown form of one of ``bases`` (an identity's recorded cases, smallest first)
    whose plan still names ``ident`` with units > grid, or None.  ``explain(list of cases) ->
    list of plan texts``."""
    for case, base in zip(bases, explain(bases)):
        g7 = g7_fields(base)
        cands = grown_candidates(case, g7[2] if g7 else 256)
        for c, plan in zip(cands, explain(cands)):
            if streams_two_units(ident, plan):
                return c
    return None


# ------------------------------------------------------------------ GPU half

def _rel(x, ref):
    return float((x.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-30))


def build_operands(sig: str, dev="cuda", aux_deriv=False, row_align=64):
    """Operands of a signature -> (a, b, out, out0, kw): ``gemm(a, b, out=out, **kw)`` is the
    product, ``out0`` the prior contents of an accumulated output.  ``row_align``: the operands'
    row stride is their columns rounded up to it (64: as production stores them; 8: the leading
    dimensions a recorded case implies, which the planner's DMA schedule choice reads)."""
    import torch

    M, N, K, a_kmaj, b_kmaj, out_f32, act, act_bwd, flags = parse_sig(sig)
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(sig.encode()))

    def r(rows, cols):
        # production operands keep 16-B aligned rows (e.g. the 64-padded vocabulary of the LM
        # head): pad the row stride and view the logical extent
        ld = (cols + row_align - 1) // row_align * row_align
        return (torch.rand(rows, ld, device=dev, generator=g) * 2 - 1).bfloat16()[:, :cols]

    a = r(M, K) if a_kmaj else r(K, M)
    b = r(N, K) if b_kmaj else r(K, N)
    odt = torch.float32 if out_f32 else torch.bfloat16
    kw = dict(a_kmaj=a_kmaj, b_kmaj=b_kmaj)
    if "b" in flags:
        kw["bias"] = torch.randn(N, device=dev, generator=g)
    if act:
        kw["act"] = act
    if "x" in flags:
        kw["aux_out"] = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    if "r" in flags:
        kw["residual"] = torch.randn(M, N, device=dev, generator=g)
    if act_bwd:
        kw["act_bwd"] = act_bwd
        kw["aux_in"] = torch.randn(M, N, device=dev, generator=g).bfloat16()
    if "c" in flags:
        kw["colsum"] = torch.zeros(N, device=dev)
    if aux_deriv:
        kw["aux_deriv"] = True
    kw["accumulate"] = "a" in flags
    out = (torch.randn(M, N, device=dev, generator=g) if kw["accumulate"] else torch.empty(M, N, device=dev)).to(odt)
    return a, b, out, (out.clone() if kw["accumulate"] else None), kw


def check_against_fp32(sig: str, a, b, out, out0, kw, label=None):
    """The product's outputs against ``_gemm_ref`` on the same bf16 operands: relative max error
    below 1.5e-2 for bf16 outputs and aux_out (2^-9 rounding), 5e-3 for f32 outputs and colsum
    (the f32 accumulation order differs over K)."""
    import torch

    from distributed_pytorch_cookbook_amd.ops.gemm import _gemm_ref

    M, N, K, a_kmaj, b_kmaj, out_f32, act, act_bwd, flags = parse_sig(sig)
    label = label or sig
    dev = out.device
    ref = out0.float() if out0 is not None else torch.empty(M, N, device=dev)
    ref_aux = torch.empty(M, N, device=dev) if "x" in flags else None
    ref_cs = torch.zeros(N, device=dev) if "c" in flags else None
    _gemm_ref(a, b, a_kmaj, b_kmaj, ref, kw.get("bias"), act, act_bwd, kw.get("aux_in"), ref_aux,
              kw.get("residual"), 1.0, None, out0 is not None, ref_cs, bool(kw.get("aux_deriv")))
    tol = 1.5e-2 if not out_f32 else 5e-3
    assert _rel(out, ref) < tol, label
    if ref_aux is not None:
        assert _rel(kw["aux_out"], ref_aux) < 1.5e-2, label + " aux_out"
    if ref_cs is not None:
        assert _rel(kw["colsum"], ref_cs) < 5e-3, label + " colsum"


@contextlib.contextmanager
def library_settings(st: dict):
    """The library-wide settings of a case (gimpl, splits, reserve, actlds, reslds), restored on exit."""
    from distributed_pytorch_cookbook_amd.ops import _lib

    lib = _lib.lib()
    try:
        _lib.set_gemm_impl(st.get("gimpl", -1))
        _lib.set_gemm_splits(st.get("splits", 0))
        _lib.set_cu_reserve(st.get("reserve", 0))
        lib.dpc_gemm7_set_act_lds(st.get("actlds", -1))
        lib.dpc_gemm7_set_res_lds(st.get("reslds", -1))
        yield
    finally:
        _lib.set_gemm_impl(-1)
        _lib.set_gemm_splits(0)
        _lib.set_cu_reserve(0)
        lib.dpc_gemm7_set_act_lds(-1)
        lib.dpc_gemm7_set_res_lds(-1)


def _case_args(args, st: dict, workspace):
    """A case's GemmArgs fields: the implementation id and the workspace, as the case states them
    (not as ops/gemm.py's table and its workspace rule would)."""
    args.impl = st.get("impl", 0)
    ws = workspace() if st.get("ws", 0) > 0 else None
    args.ws = None if ws is None else ws.data_ptr()
    args.ws_bytes = 0 if ws is None else ws.numel() * 4
    return ws


def explain_on_device(cases: list) -> list:
    """Plan texts of cases as the loaded library answers them.  Launches nothing; the pointers
    are placeholders with the alignment of real allocations."""
    from distributed_pytorch_cookbook_amd.ops import _lib

    r8 = lambda x: (x + 7) // 8 * 8  # noqa: E731
    out = []
    for case in cases:
        sig, st = parse_case(case)
        M, N, K, a_kmaj, b_kmaj, out_f32, act, act_bwd, flags = parse_sig(sig)
        a_c, b_c = (K if a_kmaj else M), (K if b_kmaj else N)
        fake = lambda slot: 0x100000000 * slot  # noqa: E731
        args = _lib.GemmArgs(
            A=fake(1), B=fake(2), C=fake(3), bias=fake(4) if "b" in flags else None,
            residual=fake(5) if "r" in flags else None, aux_in=fake(6) if act_bwd else None,
            aux_out=fake(7) if "x" in flags else None, colsum=fake(8) if "c" in flags else None,
            lda=r8(a_c), ldb=r8(b_c), ldc=N, ldr=N if "r" in flags else 0, ld_aux_in=N if act_bwd else 0,
            ld_aux_out=N if "x" in flags else 0, M=M, N=N, K=K, alpha=1.0, act=act, act_bwd=act_bwd,
            out_f32=int(out_f32), accumulate=int("a" in flags), a_kmaj=int(a_kmaj), b_kmaj=int(b_kmaj),
            a_r=M if a_kmaj else K, a_c=a_c, b_r=N if b_kmaj else K, b_c=b_c, impl=st.get("impl", 0),
            ws=fake(9) if st.get("ws", 0) > 0 else None, ws_bytes=st.get("ws", 0) << 20, aux_deriv=st.get("deriv", 0))
        with library_settings(st):
            out.append(_lib.gemm_explain(args))
    return out


def run_case(case: str, ident: str, monkeypatch, dev="cuda"):
    """Run ``case`` with its settings applied, assert that the plan the dispatcher explains for the
    call names ``ident`` and is what it launched, and compare the outputs with the fp32 reference.
    Returns the plan text."""
    import torch

    from distributed_pytorch_cookbook_amd.ops import _lib
    from distributed_pytorch_cookbook_amd.ops import gemm as gemm_mod

    sig, st = parse_case(case)
    a, b, out, out0, kw = build_operands(sig, dev, aux_deriv=bool(st.get("deriv")), row_align=8)
    plans, keep = [], []
    call = _lib.call

    def call_as_case(name, args, device=None):
        assert name == "dpc_gemm"
        keep.append(_case_args(args, st, lambda: gemm_mod._workspace(a.device)))
        plans.append(_lib.gemm_explain(args))
        call(name, args, device)
        plans.append(_lib.gemm_last_kernel())

    monkeypatch.setattr(_lib, "call", call_as_case)
    with library_settings(st):
        gemm_mod.gemm(a, b, out=out, **kw)
        torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "call", call)
    plan, last = plans
    assert KERNEL_RE.findall(plan) == [ident], (case, plan)
    assert int(plan.rsplit("last=", 1)[1]) == last, (case, plan, last)
    check_against_fp32(sig, a, b, out, out0, kw, label=case)
    return plan

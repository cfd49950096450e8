"""The GEMM dispatcher's choice, checked without a GPU.

``ops/csrc/gemm_plan.h`` is a pure host function from (arguments, settings) to a plan: which
kernel instantiation, grid, split-K plan and reduction passes a product gets.
``tests/tools/gemm_plan_tool.cpp`` prints that plan for a list of cases;
``tests/golden/gemm_plan_cases.txt`` holds the same list as the dispatcher answered it before
the planner was split out of the launch code (recorded from that dispatcher with its launches
replaced by prints).  Every production signature of ``gemm_tuned.json``, the built-in policy,
the fallbacks and the sweep switches must keep getting exactly that plan.
"""
from __future__ import annotations

import json
import os
import re
import shutil
import subprocess

import pytest

import gemm_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = os.path.join(ROOT, "distributed_pytorch_cookbook_amd", "ops")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_cases.txt")
WS = " ws=1024"  # MiB: the default workspace of ops/gemm.py

LAYOUTS = ("kk", "km", "mm", "mk")
# plain and fused calls of tests/test_kernels_gpu.py (test_gemm_v7_v8_v9, the act-gradient,
# residual and aux_deriv tests), as signature tails <out>:<act><act_bwd>:<flags>
EPILOGUES = ("h:00:", "f:00:", "f:00:a", "f:21:bxrc", "h:02:c", "h:03:c", "f:02:", "h:20:bx", "h:20:bx deriv=1",
             "f:20:bxr", "f:00:br", "f:10:xr")
RAGGED = ((300, 264, 96), (300, 264, 128), (257, 520, 1000), (77, 1000, 1023), (1023, 768, 768), (4096, 4352, 256),
          (130, 136, 4160))


def candidates() -> tuple:
    src = open(os.path.join(OPS, "gemm.py")).read()
    return tuple(int(v) for v in re.search(r"^_CANDIDATES = \(([^)]*)\)", src, re.M).group(1).split(","))


def table() -> dict:
    with open(os.path.join(OPS, "gemm_tuned.json")) as f:
        return json.load(f)["impl"]


def _ws(sig: str) -> str:
    """ops/gemm.py passes the workspace to plain f32 products and to act' + column-sum ones."""
    _, _, out, acts, flags = sig.split(" ")[0].split(":")
    return WS if (out == "f" and acts == "00" and flags in ("", "a")) or ("c" in flags and acts[1] != "0") else ""


def cases() -> list:
    """The case list of the golden file, in its order (tests/tools/gemm_plan_tool.cpp has the format)."""
    out = []
    tab = table()
    sigs = sorted(tab)
    # every production signature with its table entry, with and without the workspace, and under
    # the built-in policy
    for sig in sigs:
        out += [f"{sig} impl={tab[sig]}{WS}", f"{sig} impl={tab[sig]}", f"{sig}{_ws(sig)}"]
    # every class of the table x every candidate, at the class's smallest and largest shape
    classes = {}
    for sig in sigs:
        classes.setdefault(sig.split(":", 1)[1], []).append(sig)

    def volume(sig):
        m, n, k = (int(v) for v in sig.split(":")[0].split("x"))
        return (m * n * k, sig)

    cand = candidates()
    ends = {cls: tuple(dict.fromkeys((min(v, key=volume), max(v, key=volume)))) for cls, v in sorted(classes.items())}
    for cls, pair in ends.items():
        out += [f"{sig} impl={impl}{_ws(sig)}" for sig in pair for impl in cand[1:]]
    # ragged and odd shapes, every layout, plain and fused, under the policy; v8 and v7 on the smallest
    for M, N, K in RAGGED:
        out += [f"{M}x{N}x{K}:{lay}:{epi}{_ws(':' + lay + ':' + epi)}" for lay in LAYOUTS for epi in EPILOGUES]
    out += [f"300x264x96:{lay}:{epi}{_ws(':' + lay + ':' + epi)} gimpl={impl}" for lay in LAYOUTS for epi in EPILOGUES
            for impl in (21, 25)]
    # the plain product under every id: K % 64 != 0 (no v9), and leading dimensions too short for
    # the grouped DMA schedules (pairs need 1 KiB of rows before a piece, quads 3 KiB); those also
    # fused and split, v7 and v8
    for lay in LAYOUTS:
        out += [f"{dims}:{lay}:h:00: gimpl={impl}" for dims in ("300x264x96", "72x72x32") for impl in cand[1:]]
        out += [f"72x72x64:{lay}:{epi} gimpl={impl}" for epi in EPILOGUES[1:] for impl in (20, 21)]
        out += [f"{dims}:{lay}:f:00: gimpl={impl} splits=2{ws}" for dims in ("72x72x4096", "600x520x8192")
                for impl in (20, 21) for ws in (WS, "")]
    # requirement failures, one at a time
    for forced in ("", " gimpl=20", " gimpl=26"):
        out += [bad + forced for bad in (
            "1024x768x768:kk:h:00: coff=8", "1024x768x768:kk:h:00: ldc=772", "1024x768x768:km:h:02:c ldi=772",
            "1024x768x32:kk:h:00:", "1024x772x768:kk:h:00:", "1024x770x768:kk:h:00:", "1024x768x768:kk:h:00: ac=704",
            "1024x768x768:kk:h:00: bc=704", "1024x768x784:kk:h:00:", "1024x768x768:kk:h:20:bx ldo=772")]
    # forced split counts (test_gemm_forced_split_k)
    for dims in ("77x1000x4160", "600x520x8192", "2304x136x4096"):
        out += [f"{dims}:mm:f:00:{acc} gimpl={impl} splits={splits}{ws}" for impl in (2, 10, 16, 21, 26)
                for splits in (2, 3, 8) for acc, ws in (("a", WS), ("", ""))]
        out.append(f"{dims}:mm:f:00: gimpl=2 splits=3 xcd=1")
    # CUs reserved for a collective in flight
    for cls, pair in ends.items():
        out += [f"{sig} impl={tab[sig]}{_ws(sig)} reserve={r}" for sig in pair for r in (16, 200)]
    # the LDS-staged epilogues switched off, another store policy, aux_deriv, v7d
    for dims in ("1023x768x768", "300x264x96", "4096x4352x256"):
        for lay in LAYOUTS[:3]:
            out += [f"{dims}:{lay}:h:0{actb}:c{ws} gimpl=25{sw}" for actb in (2, 3) for ws in (WS, "")
                    for sw in (" actlds=0", " nt=3", " nt=3 actlds=0")]
        out += [f"{dims}:{lay}:{epi} gimpl=25{sw}" for lay in LAYOUTS[:2] for epi in EPILOGUES[9:]
                for sw in (" reslds=0", " nt=3")]
        out += [f"{dims}:kk:{epi} nt=3" for epi in ("h:00:", "f:00:", "h:20:bx")]
    for dims in ("1023x768x768", "4096x4352x256", "300x264x192", "2048x3072x768"):
        for impl in (26, 25, 21, 10, 2):
            out += [f"{dims}:kk:h:20:bx deriv=1 gimpl={impl}", f"{dims}:km:h:03:c{WS} gimpl={impl}"]
    out += ["1024x768x768:kk:h:00:x deriv=1", "1024x768x768:kk:h:20:b deriv=1"]  # aux_deriv without GELU + aux_out
    for dims in ("16000x3072x768", "10000x2048x576", "65472x768x3072", "4096x4352x512"):
        out += [f"{dims}:{call} gimpl=24" for call in ("kk:h:20:bx", f"km:h:02:c{WS}", "kk:f:20:bxr", "kk:h:20:bx deriv=1",
                                                       "km:h:03:c", "kk:h:00:")]
    # an mn-major operand stored with fewer columns than the product has rows (A) or columns (B):
    # the descriptor-bounded loads would read what follows the stored columns, so the
    # register-staged kernel runs it, whatever is forced (tests/gemm_forms.py: short_a_mn, short_b_mn)
    for forced in ("", " gimpl=2", " gimpl=10", " gimpl=20", " gimpl=26"):
        out += [short + forced for short in ("96x264x192:mk:h:00: ac=77", "96x264x192:mm:f:00: ac=72" + WS,
                                             "77x96x192:km:h:00: bc=72", "77x96x192:km:f:00: bc=77" + WS)]
    return list(dict.fromkeys(out))  # (a few cases belong to two groups)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("plan") / "gemm_plan_tool"
    src = os.path.join(ROOT, "tests", "tools", "gemm_plan_tool.cpp")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(OPS, "csrc"), src, "-o", str(exe)], check=True)
    return str(exe)


def _golden() -> list:
    with open(GOLDEN) as f:
        return [ln.rstrip("\n") for ln in f if ln.strip()]


def test_plans_match_recorded_dispatcher(tool):
    r = subprocess.run([tool], input="\n".join(cases()) + "\n", capture_output=True, text=True, check=True)
    got, want = r.stdout.splitlines(), _golden()
    assert [g.split("\t")[0] for g in got] == [w.split("\t")[0] for w in want], "case list differs from the golden file"
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, f"{len(bad)} plans differ, e.g.\n got  {bad[0][0]}\n want {bad[0][1]}"


def test_candidates_are_the_table(tool):
    r = subprocess.run([tool, "--impls"], capture_output=True, text=True, check=True)
    ids = {int(ln.split("\t")[0]) for ln in r.stdout.splitlines()}
    cand = set(candidates())
    assert cand - {0} <= ids  # (0 = the built-in policy)
    assert ids - {1} <= cand  # (1 = the fallback only)
    assert set(table().values()) <= cand


def test_every_compiled_kernel_is_reached():
    """The persistent-family instantiations compiled in the part files are exactly the ones some
    recorded plan names: none dead, none missing."""
    with open(os.path.join(OPS, "csrc", "gemm_parts.txt")) as f:
        compiled = {ln.strip() for ln in f if ln.strip() and not ln.startswith("#")}
    named = set(re.findall(r"gemm(?:7|7d|9)_kernel<[^>]*>", "\n".join(w.split("\t")[1] for w in _golden())))
    assert named == compiled, (sorted(compiled - named), sorted(named - compiled))


def test_every_compiled_kernel_has_gpu_cases(tool):
    """The case table of test_gemm_instantiations_gpu.py covers every line of gemm_parts.txt:
    each identity has a recorded case that a running process can set up, and a grown form of one
    in which a workgroup streams at least two units while the plan still names that identity."""
    def explain(cs):
        r = subprocess.run([tool], input="\n".join(cs) + "\n", capture_output=True, text=True, check=True)
        return [ln.split("\t")[1] for ln in r.stdout.splitlines()]

    by = gemm_cases.cases_by_identity()
    idents = gemm_cases.identities()
    assert not [i for i in idents if i not in by]
    assert explain([by[i][0] for i in idents]) == [dict(gemm_cases.golden())[by[i][0]] for i in idents]
    two = {i: gemm_cases.two_unit_case(i, by[i], explain) for i in idents}
    assert not [i for i in idents if two[i] is None]

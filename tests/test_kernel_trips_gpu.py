"""Loop trips of the memory-bound kernels that no small shape reaches, the loss-scaling kernels,
and the run structure of the embedding backward (cases and shared checks: tests/mem_cases.py).

* LayerNorm backward with more than one row per wave (the persistent grid pinned to its minimum),
  so the row-prefetch kernel alternates its two row buffers and leaves through either ``break``;
* AdamW, the f32 -> bf16 cast, dropout_residual and amp_check past the grid cap of
  ``grid_for`` (misc.hip), where a thread takes a second trip;
* amp_check / amp_update against torch's GradScaler rule, eagerly and replayed from a graph;
* the sorted embedding backward on layouts that meet every chunk phase and piece length, and the
  atomic one (D > 2048) against the same per-table references."""
import pytest
import torch

import mem_cases as mc
from kernel_checks import MARGIN, assert_elem_bound, assert_guards_intact, assert_local_close, guarded
from test_kernel_edges_gpu import _adam64, _ld, check_layernorm_bwd

from distributed_pytorch_cookbook_amd.ops import _lib
from distributed_pytorch_cookbook_amd.ops import embedding as emb
from distributed_pytorch_cookbook_amd.ops.amp import GradScaler
from distributed_pytorch_cookbook_amd.ops.dropout import DropSpec, dropout_residual, keep_mask
from distributed_pytorch_cookbook_amd.ops.elementwise import cast_f32_bf16
from distributed_pytorch_cookbook_amd.ops.embedding import embedding_bwd
from distributed_pytorch_cookbook_amd.ops.optim import FlatAdamW

pytestmark = pytest.mark.gpu
dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture
def native_calls(monkeypatch):
    """The names of the native entry points called through ops._lib.call, in order."""
    names = []
    real = _lib.call

    def counting(name, args, device=None):
        names.append(name)
        return real(name, args, device)

    monkeypatch.setattr(_lib, "call", counting)
    return names


# ---------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("dy_bf16", [False, True])
@pytest.mark.parametrize("pf", [1, 0])
@pytest.mark.parametrize("D", [100, 1024])
@pytest.mark.parametrize("T", [mc.ln_bwd_sweep_rows + 2, 2 * mc.ln_bwd_sweep_rows + 3])
def test_layernorm_bwd_trips(T, D, pf, dy_bf16):
    """The checks of test_layernorm_bwd_edges with the grid pinned to 256 workgroups (the
    smallest the dispatcher launches: 1024 rows per sweep).  T = 1026: waves 0 and 1 of workgroup
    0 do two rows, every other wave one; T = 2051: two or three.  With pf = 1 a wave's last row
    is computed from the second buffer (two rows) or from the first again (three), and each
    prefetch past the end re-reads row T - 1."""
    assert mc.ln_bwd_rows_per_wave(T) == ((1, 2) if T < 2 * mc.ln_bwd_sweep_rows else (2, 3))
    check_layernorm_bwd(T, D, pf, dy_bf16, blocks=mc.LN_BWD_MIN_BLOCKS)


# ---------------------------------------------------------------- flat kernels past the grid cap
def test_adamw_trips():
    """n = 4 (2 x 8192 x 256 + 300): every thread's first trip moves two vectors, and 300 threads
    take a second trip with the second vector past the end (``has1`` false).  Two steps against
    f64 AdamW, param within 4 ulp, shadow == bf16(param), both moments written everywhere."""
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    n = 4 * (2 * mc.FLAT_MAX_BLOCKS * mc.FLAT_BLOCK + 300)
    assert mc.flat_trips(n // 4, vecs_per_trip=2) == 2
    torch.manual_seed(n)
    p0 = torch.randn(n, device=dev)
    p0 = torch.where(p0 >= 0, p0 + 0.5, p0 - 0.5)  # (|param| >= 0.5: see test_adamw_subrange_edges)
    p = guarded(n, F32, dev, fill=p0)
    g = guarded(n, F32, dev, fill=0.0)
    sh = guarded(n, BF, dev, fill=7.0)
    opt = FlatAdamW(p, g, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, shadow=sh)
    opt.exp_avg = guarded(n, F32, dev, fill=0.0)
    opt.exp_avg_sq = guarded(n, F32, dev, fill=0.0)
    p64 = p0.double()
    m64, v64 = torch.zeros_like(p64), torch.zeros_like(p64)
    del p0
    for step in (1, 2):
        g.normal_()
        opt.step()
        p64, m64, v64 = _adam64(p64, m64, v64, g.double(), step, lr, b1, b2, eps, wd)
    assert_elem_bound(p, p64, 4 * 2.0 ** -23 * p64.abs(), what="param", family="adamw (fraction of 4 ulp)")
    assert torch.equal(sh.view(torch.int16), p.bfloat16().view(torch.int16))
    assert (opt.exp_avg != 0).all() and (opt.exp_avg_sq != 0).all()
    assert_guards_intact(p, g, sh, opt.exp_avg, opt.exp_avg_sq)


def test_cast_trips():
    n = 4 * (mc.FLAT_MAX_BLOCKS * mc.FLAT_BLOCK + 300)
    assert mc.flat_trips(n // 4) == 2
    torch.manual_seed(n)
    src = torch.randn(n, device=dev)
    dst = guarded(n, BF, dev)
    cast_f32_bf16(src, dst)
    assert torch.equal(dst.view(torch.int16), src.bfloat16().view(torch.int16))
    assert_guards_intact(dst)


def test_dropout_residual_trips():
    """T = 2049, N = 4100: 2,100,225 vectors, 3,073 more than one trip of the capped grid."""
    torch.manual_seed(13)
    T, N = 2049, 4100
    assert mc.flat_trips(T * (N // 4)) == 2
    spec = DropSpec.make(0.1, seed=(5 << 32) | 17, site=9)
    y, r = torch.randn(T, N, device=dev), torch.randn(T, N, device=dev)
    out = guarded((T, N), F32, dev, ld=_ld(N))
    dropout_residual(y, r, spec, out=out)
    keep = keep_mask(spec, T, N, dev)
    assert_local_close(out, r.double() + y.double() * keep.double(), r + y * keep, MARGIN, axes="rows",
                       what="dropout_residual", family="elementwise")
    assert torch.equal(out == r, (keep == 0) | (y == 0))
    assert_guards_intact(out)


# ---------------------------------------------------------------- loss scaling
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("n", mc.AMP_SMALL + [mc.AMP_LARGE])
def test_amp_check(n, offset, native_calls):
    """GradScaler.check on a flat buffer inside guard bands of quiet NaNs -- a kernel that read
    one element outside [0, n) would raise the flag on clean data -- over the matrix of
    mem_cases.check_amp_matrix.  A buffer whose base is one element past a 16-B boundary
    (``offset``) gives the same answers through the torch path; the aligned one must have run the
    kernel, once per check."""
    sc = GradScaler(dev)
    g = guarded(n, F32, dev, offset=offset)
    mc.amp_clean_fill(g)
    checks = mc.check_amp_matrix(sc, g)
    assert native_calls.count("dpc_amp_check") == (0 if offset else checks)
    sc.check(g[:0])  # n == 0 launches nothing
    assert native_calls.count("dpc_amp_check") == (0 if offset else checks) and float(sc.found_inf) == 0.0
    assert_guards_intact(g)


def _run_script(sc, script, exact_inv):
    pattern, _, _, states = script
    for i, found in enumerate(pattern):
        sc.found_inf.fill_(float(found))
        sc.update()
        mc.check_scaler_state(sc, states[i], exact_inv, what=f"step {i}")


@pytest.mark.parametrize("growth,backoff", [(2.0, 0.5), (1.7, 0.6)])
def test_amp_update_follows_the_script(growth, backoff, native_calls):
    """amp_update_kernel over mem_cases.scaler_script (12 steps, interval 3: two growths, three
    back-offs, one of them right after a growth).  Powers of two: inv_scale bit-equal to 1 / scale;
    growth 1.7 / backoff 0.6: within 2^-22 relative of the f64 reciprocal."""
    script = mc.scaler_script(growth, backoff)
    sc = GradScaler(dev, init_scale=script[2], growth_factor=growth, backoff_factor=backoff,
                    growth_interval=script[1])
    _run_script(sc, script, exact_inv=(growth, backoff) == (2.0, 0.5))
    assert native_calls.count("dpc_amp_update") == len(script[0])


def test_amp_check_update_replayed_from_a_graph(native_calls):
    """check(g); update() captured once (a sequential chain, as the engines record it) and
    replayed over the first six steps of the script; g is poisoned or cleaned between replays and
    the state is read only after each replay."""
    pattern, interval, init, states = mc.scaler_script()
    sc = GradScaler(dev, init_scale=init, growth_interval=interval)
    n = 1027
    g = guarded(n, F32, dev)
    mc.amp_clean_fill(g)
    clean = g.clone()
    warm = GradScaler(dev)  # both kernels have run once before anything is recorded
    warm.check(g)
    warm.update()
    torch.cuda.synchronize()
    del native_calls[:]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sc.check(g)
        sc.update()
    assert native_calls == ["dpc_amp_check", "dpc_amp_update"]
    assert float(sc.scale_t) == init and float(sc.tracker) == 0.0  # capture ran nothing
    poison_at = {2: (n - 1, float("nan"))}  # the script's first overflow: the scalar tail
    assert [i for i, f in enumerate(pattern[:6]) if f] == sorted(poison_at)
    for i in range(6):
        g.copy_(clean)
        if i in poison_at:
            at, v = poison_at[i]
            g[at] = v
        graph.replay()
        torch.cuda.synchronize()
        mc.check_scaler_state(sc, states[i], exact_inv=True, what=f"replay {i}")
    assert len(native_calls) == 2
    assert_guards_intact(g)


# ---------------------------------------------------------------- embedding backward
def _emb_case(L, D, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    dout = torch.randn(L["T"], D, device=dev, generator=g)
    bt = torch.randn(L["V"], D, device=dev, generator=g)
    bp = torch.randn(L["P"], D, device=dev, generator=g)
    return dout, bt, bp, L["ids"].to(dev), L["pos"].to(dev)


def _emb_run(dout, ids, pos, bt, bp, with_tok=True, with_pos=True):
    dt = guarded(bt.shape, F32, dev, fill=bt) if with_tok else None
    dp = guarded(bp.shape, F32, dev, fill=bp) if with_pos else None
    embedding_bwd(dout, ids, pos, dt, dp)
    return dt, dp


def _emb_check(dt, dp, dout, ids, pos, bt, bp, family):
    if dt is not None:
        mc.check_embedding_table(dt, bt, dout, ids, "dtok", family)
        assert_guards_intact(dt)
    if dp is not None:
        mc.check_embedding_table(dp, bp, dout, pos, "dpos", family)
        assert_guards_intact(dp)


@pytest.mark.parametrize("D", [4, 260, 1024, 1280, 1300, 2048])  # NV 1, 2, 4 (8-row groups), 5, 6, 8 (4-row groups)
@pytest.mark.parametrize("variant", [0, 1])
def test_embedding_bwd_sorted_runs(variant, D, native_calls):
    """The sorted path on the layouts of mem_cases.run_layout (every chunk phase and piece length;
    T = 372 with a partial last chunk, T = 376 with a run that ends on the last chunk's end), the
    token table with three out-of-range ids.  Unnamed rows bit-unchanged, named rows within the
    f32 index_add's floor, and a second call from the same state bit-identical."""
    L = mc.run_layout(variant)
    dout, bt, bp, ids, pos = _emb_case(L, D, 1000 * D + variant)
    dt, dp = _emb_run(dout, ids, pos, bt, bp)
    assert native_calls == ["dpc_embedding_bwd_sorted"] and emb._ws.get(torch.cuda.current_device()) is not None
    _emb_check(dt, dp, dout, ids, pos, bt, bp, "embedding bwd sorted")
    dt2, dp2 = _emb_run(dout, ids, pos, bt, bp)
    assert torch.equal(dt.view(torch.int32), dt2.view(torch.int32))
    assert torch.equal(dp.view(torch.int32), dp2.view(torch.int32))


def _small_emb_layout():
    """T = 21 rows over V = 37 tokens and 7 positions; three ids and (on another row) one position
    out of range: each table leaves out the rows whose own index is bad, and only those."""
    V, P, T = 37, 7, 21
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V, (T,), generator=g)
    ids[3], ids[10], ids[20] = V + 3, -1, 2 ** 40
    pos = torch.arange(P).repeat(3)
    pos[5] = P + 2
    return dict(T=T, V=V, P=P, ids=ids, pos=pos)


def test_embedding_bwd_atomic(native_calls):
    """The atomic scatter (misc.hip: emb_bwd_kernel; D = 2052 is past the sorted path's widest
    row) against the same per-table references as the sorted path: a row with a bad id still adds
    to its position row, a row with a bad position still adds to its token row."""
    L = _small_emb_layout()
    dout, bt, bp, ids, pos = _emb_case(L, 2052, 77)
    dt, dp = _emb_run(dout, ids, pos, bt, bp)
    assert native_calls == ["dpc_embedding_bwd"]
    _emb_check(dt, dp, dout, ids, pos, bt, bp, "embedding bwd atomic")


@pytest.mark.parametrize("D,entry", [(260, "dpc_embedding_bwd_sorted"), (2052, "dpc_embedding_bwd")])
@pytest.mark.parametrize("which", ["tok", "pos"])
def test_embedding_bwd_one_table(which, D, entry, native_calls):
    """dtok=None and dpos=None, on both paths."""
    L = mc.run_layout(0) if D <= 2048 else _small_emb_layout()
    dout, bt, bp, ids, pos = _emb_case(L, D, D)
    dt, dp = _emb_run(dout, ids, pos, bt, bp, with_tok=which == "tok", with_pos=which == "pos")
    assert native_calls == [entry] and (dt is None) == (which == "pos") and (dp is None) == (which == "tok")
    _emb_check(dt, dp, dout, ids, pos, bt, bp, "embedding bwd one table")

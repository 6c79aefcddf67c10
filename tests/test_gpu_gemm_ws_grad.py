"""phc_twin_gemm's wave-specialised persistent grid (phc_gemm.hip kWsTile / kWsGrad) against the
one-tile-per-workgroup kernel of the same launch, bit for bit (needs an MI355X).

The reference of every case is the same call with max_workgroups = 10**6: the grid equals the tile
count and no persistent loop runs.  phc_twin_gemm_plan says which kernel a call takes, so every case
also pins that it runs the kernel it is written for: 256 x 256 tiles are chosen from 256 tiles up,
which is why every shape here has at least that many.  Outputs and bias_grad are pre-filled with a
sentinel, so an element no thread wrote shows.

Tolerances against float64 torch (the silu'-aux input gradient out = (g W) * aux): those of
test_gpu_gemm.py::test_silu_deriv_aux_pair — one rounding of the output type on top of fp32
accumulation (rel. 2^-8 f16, 2^-5 bf16, abs 5e-3), bias-gradient sums rel. 2e-2, abs 0.5.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ONE_TILE = 10 ** 6
SENTINEL = 7.0


def _split(t):
    """GROUPED [2, m, n] -> SPLIT [m, 2 n]."""
    return t.permute(1, 0, 2).reshape(t.shape[1], -1).contiguous()


def _grouped(t, n):
    """SPLIT [m, 2 n] -> GROUPED [2, m, n] (a view)."""
    return t.view(t.shape[0], 2, n).permute(1, 0, 2)


@functools.lru_cache(maxsize=None)
def _grad_case(dtype, m, n, k, aux_dtype=None):
    """Operands of an input-gradient launch, batch 2, and its float64 result (GROUPED); shared by the
    cases that use the shape, never written."""
    g = torch.Generator(device=DEV).manual_seed(21)
    gr = (torch.randn((2, m, k), device=DEV, generator=g) * 0.5).to(dtype)
    wt = (torch.randn((2, n, k), device=DEV, generator=g) / k ** 0.5).to(dtype)
    aux = (torch.rand((2, m, n), device=DEV, generator=g) * 1.2 - 0.1).to(aux_dtype or dtype)  # silu' lies in (-0.1, 1.1)
    ref = torch.bmm(gr.double(), wt.double().transpose(1, 2)) * aux.double()
    return gr, wt, aux, ref


def _run_grad(N, gr, wt, aux, layout, max_workgroups, want_ws=None, want_grid=None):
    _, m, _ = gr.shape
    n = wt.shape[1]
    shape = (m, 2 * n) if layout == N.SPLIT else (2, m, n)
    aux_l = _split(aux) if layout == N.SPLIT else aux
    out = torch.full(shape, SENTINEL, dtype=gr.dtype, device=DEV)
    db = torch.full((2 * n,), -12345.0, device=DEV)
    kw = dict(aux=aux_l, aux_layout=layout, out_layout=layout, max_workgroups=max_workgroups)
    plan = N.twin_gemm_plan(gr, wt, N.EPI_DSILU_GRAD, out, (2, n), **kw)
    assert plan["tile"] == 256
    if want_ws is not None:
        assert plan["wave_specialised"] == want_ws, plan
    if want_grid is not None:
        assert plan["grid"] == want_grid, plan
    N.twin_gemm(gr, wt, N.EPI_DSILU_GRAD, out, (2, n), bias_grad=db, **kw)
    return (_grouped(out, n) if layout == N.SPLIT else out), db


def _check_f64(out, db, ref):
    """out and bias_grad against the float64 result (the module docstring's tolerances)."""
    tol = 2.0 ** -8 if out.dtype == torch.float16 else 2.0 ** -5
    torch.testing.assert_close(out.double(), ref, rtol=tol, atol=5e-3)
    torch.testing.assert_close(db.double(), ref.sum(1).reshape(-1), rtol=2e-2, atol=0.5)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("k", [128, 192])  # 2 and 3 K-steps: the last K-step reads either operand buffer
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_dsilu_grad_whole_tiles(dtype, k, layout):
    """DSILU_GRAD in its role copies (37 workgroups over 256 whole tiles, a ragged last step): out and
    bias_grad equal the one-tile kernel's bit for bit, in both twin layouts; out also against float64."""
    from puffer_phc_amd import _native as N

    m, n = 16384, 512
    gr, wt, aux, ref = _grad_case(dtype, m, n, k)
    out1, db1 = _run_grad(N, gr, wt, aux, layout, ONE_TILE, want_ws=False, want_grid=256)
    out, db = _run_grad(N, gr, wt, aux, layout, 37, want_ws=True, want_grid=37)
    assert torch.equal(out, out1)
    assert torch.equal(db, db1)
    _check_f64(out, db, ref)


def test_dsilu_grad_automatic_grid():
    """More tiles (260) than CUs: the default launch is one wave-specialised workgroup per CU."""
    from puffer_phc_amd import _native as N

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus < 260
    gr, wt, aux, ref = _grad_case(torch.float16, 16640, 512, 128)
    out1, db1 = _run_grad(N, gr, wt, aux, N.GROUPED, ONE_TILE, want_ws=False, want_grid=260)
    out, db = _run_grad(N, gr, wt, aux, N.GROUPED, 0, want_ws=True, want_grid=cus)
    assert torch.equal(out, out1)
    assert torch.equal(db, db1)
    _check_f64(out, db, ref)


@pytest.mark.parametrize("case", ["ragged", "aux_f32"])
def test_dsilu_grad_fallback(case):
    """Ragged tiles, or an fp32 aux: the generic persistent copy, still the one-tile result."""
    from puffer_phc_amd import _native as N

    if case == "ragged":
        gr, wt, aux, ref = _grad_case(torch.float16, 16384 + 77, 700, 128)
    else:
        gr, wt, aux, ref = _grad_case(torch.float16, 16384, 512, 128, torch.float32)
    out1, db1 = _run_grad(N, gr, wt, aux, N.GROUPED, ONE_TILE, want_ws=False)
    out, db = _run_grad(N, gr, wt, aux, N.GROUPED, 37, want_ws=False, want_grid=37)
    assert torch.equal(out, out1)
    assert torch.equal(db, db1)
    _check_f64(out, db, ref)


@functools.lru_cache(maxsize=None)
def _fwd_case(dtype, m, n):
    g = torch.Generator(device=DEV).manual_seed(22)
    k = 192
    a = torch.randn((2, m, k), device=DEV, generator=g).to(dtype)
    w = (torch.randn((2, n, k), device=DEV, generator=g) / k ** 0.5).to(dtype)
    bias = torch.randn(2 * n, device=DEV, generator=g)
    return a, w, bias


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("epi", ["bias_silu_d", "bias_silu", "bias_f32"])
@pytest.mark.parametrize("shape", [(16461, 700), (16640, 768)])  # 390 tiles of 256 x 256: ragged, whole
def test_forward_wave_specialised_matches_one_tile(dtype, epi, shape):
    """The forward epilogues at shapes that do take 256 x 256 tiles: 37 wave-specialised workgroups
    against the one-tile kernel, output and aux bit for bit."""
    from puffer_phc_amd import _native as N

    m, n = shape
    a, w, bias = _fwd_case(dtype, m, n)
    ep = {"bias_silu_d": N.EPI_BIAS_SILU_D, "bias_silu": N.EPI_BIAS_SILU, "bias_f32": N.EPI_BIAS}[epi]
    odt = torch.float32 if epi == "bias_f32" else dtype
    outs = []
    for mwg, ws in ((ONE_TILE, False), (37, True)):
        out = torch.full((2, m, n), SENTINEL, dtype=odt, device=DEV)
        aux = None if epi == "bias_f32" else torch.full((2, m, n), SENTINEL, dtype=dtype, device=DEV)
        plan = N.twin_gemm_plan(a, w, ep, out, (2, n), bias=bias, aux=aux, max_workgroups=mwg)
        assert plan == {"tile": 256, "grid": 390 if mwg == ONE_TILE else 37, "wave_specialised": ws}
        N.twin_gemm(a, w, ep, out, (2, n), bias=bias, aux=aux, max_workgroups=mwg)
        outs.append((out, aux))
    assert torch.equal(outs[1][0], outs[0][0])
    if outs[0][1] is not None:
        assert torch.equal(outs[1][1], outs[0][1])
    assert not bool((outs[0][0] == SENTINEL).all(-1).any())

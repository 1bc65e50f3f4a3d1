"""The error bound of the pruned PointNet max, on the CPU: tests/pointnet_prune_cases.py models the bound pass in
torch with the engine's constants (bf16 planes by .bfloat16().float(), products accumulated in float32).  For every input class
each row that holds a channel's maximum -- by the fp32 reference relu(fma(a @ w^T, scale, shift)) and by the same in float64 --
must be a candidate, under the tightest thresholds a launch can end with (those of all rows; a kernel tests against older, lower
ones and flags no less).  A channel whose maximum is 0 needs no candidate: the result starts from zero.  For the plain random class
the candidates under the seed launch's thresholds (every 4th row tile, the loosest the main launch starts from) must fit the
slots the engine reserves."""
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import engine as E
from tests import pointnet_prune_cases as PC

# (N, K, C): many rows per channel, where pruning pays, and the real widths of conv5
SHAPES = [(4096, 64, 64), (1024, 512, 1024)]


def _references(a, w, scale, shift):
    f32 = torch.relu(((a @ w.t()).double() * scale.double() + shift.double()).float())
    f64 = torch.relu(a.double() @ w.double().t() * scale.double() + shift.double())
    return f32, f64


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", PC.CPU_CLASSES)
def test_every_winner_is_a_candidate(kind, shape):
    N, K, C = shape
    a, w, scale, shift = PC.make_case(kind, 1, N, K, C)
    ub, lb = PC.bounds(a, w, scale, shift)
    cand = PC.flagged(ub, PC.thresholds(lb, torch.ones(N, dtype=torch.bool)))
    for ref in _references(a, w, scale, shift):
        top = ref.amax(0)
        winners = (ref == top[None, :]) & (top > 0)[None, :]
        assert winners.any(0).sum() == (top > 0).sum()
        missed = winners & ~cand
        assert not missed.any(), f"{int(missed.sum())} winners of {ref.dtype} are no candidates"
    if kind == "dup50":                              # ties: all copies of a winner row are candidates (N // base rows copies at least)
        assert int(cand.sum(0)[top > 0].min()) >= N // -(-N // 50)
    if kind == "neg_channel":
        assert not cand[:, 0].any() and not cand[:, C - 1].any()


def test_random_rows_fit_the_reserved_slots():
    N, K, C = SHAPES[0]
    a, w, scale, shift = PC.make_case("random", 1, N, K, C)
    ub, lb = PC.bounds(a, w, scale, shift)
    seed_rows = (torch.arange(N) // 64) % E.PRUNE_SEED_STRIDE == 0           # Cout <= 64: 64-row tiles
    rows = PC.flagged(ub, PC.thresholds(lb, seed_rows)).any(1)
    assert 0 < int(rows.sum()) < E.prune_cap(N) < N
    # a maximum over a quarter of the rows is exceeded by ~ k rows per channel: far from the slots
    assert int(rows.sum()) <= 2 * E.PRUNE_SEED_STRIDE * C


def test_bound_constants():
    assert E.prune_cap(35000) == 5632 and E.prune_cap(4096) == 768
    assert E.prune_rel(512) == 4 * 2.0 ** -18 + 7 * 512 * 2.0 ** -24
    w = torch.ones(2, 64)
    g = E.prune_bound_g(w, torch.tensor([1.0, -2.0]), 64)
    exact = E.prune_rel(64) * 8.0
    assert g.dtype == torch.float32 and exact < float(g[0]) < exact * 1.002 and 2 * exact < float(g[1]) < 2 * exact * 1.002

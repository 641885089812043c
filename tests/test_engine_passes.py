"""The passes of the engine's chunked per-point queries (lcgp_amd.engine.point_passes): host only, no GPU and no library.
The one place that holds the rule behind "results are bitwise independent of PREDICT_CHUNK": a pass never runs below 128
rows while n0 has them, and a short last pass is moved back over its predecessor."""
import pytest

from lcgp_amd.engine import point_passes

N0S = list(range(1, 701)) + [2048, 2100, 4148]
PREDICT_CHUNKS = (1, 64, 100, 128, 129, 200, 400, 2048)
DIMS = (1, 2, 3, 7)


def _plain_chunks(n0):
    """predict / predict_grad / predict_param_grad"""
    return sorted({min(n0, c) for c in PREDICT_CHUNKS})


def _tile_chunks(n0):
    """predict_hess / predict_grad_cov (PREDICT_CHUNK // d) and predict_marginal (d = 1)"""
    return sorted({min(n0, max(128, c // d)) for c in PREDICT_CHUNKS for d in DIMS})


def test_plain_passes_are_the_range_loop():
    for n0 in N0S:
        for chunk in _plain_chunks(n0):
            assert point_passes(n0, chunk, False) == [(lo, min(chunk, n0 - lo), lo) for lo in range(0, n0, chunk)]


def test_tile_passes_stay_inside_and_keep_128_rows():
    for n0 in N0S:
        for chunk in _tile_chunks(n0):
            passes = point_passes(n0, chunk, True)
            assert len(passes) == -(-n0 // chunk)
            for lo, rows, fresh in passes:
                assert rows <= chunk and 0 <= lo <= fresh < lo + rows <= n0
                assert rows >= 128 or n0 < 128


def test_tile_passes_cover_every_row_once():
    """[fresh, lo + rows) partitions 0 .. n0: the weighted sum of grad_cov_block counts no row twice"""
    for n0 in N0S:
        for chunk in _tile_chunks(n0):
            end = 0
            for lo, rows, fresh in point_passes(n0, chunk, True):
                assert fresh == end
                end = lo + rows
            assert end == n0


def test_only_a_short_last_pass_moves_back():
    for n0 in N0S:
        for chunk in _tile_chunks(n0):
            passes = point_passes(n0, chunk, True)
            plain = point_passes(n0, chunk, False)
            assert passes[:-1] == plain[:-1]
            if plain[-1][1] >= 128 or n0 < 128:
                assert passes[-1] == plain[-1]
            else:
                assert passes[-1] == (n0 - 128, 128, plain[-1][0])


@pytest.mark.parametrize("n0, chunk, want", [
    (300, 128, [(0, 128, 0), (128, 128, 128), (172, 128, 256)]),
    (100, 100, [(0, 100, 0)]),
    (128, 128, [(0, 128, 0)]),
    (129, 128, [(0, 128, 0), (1, 128, 128)]),
])
def test_literal_cases(n0, chunk, want):
    assert point_passes(n0, chunk, True) == want

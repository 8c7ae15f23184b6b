"""The column store's catch-up (mfgp_lattice.inl: k_vcol_build), its index map restated
on the host: V is stored [tile][row][64 cells] (element (i, c) at (c // 64) vld 64 +
i 64 + c % 64), the store Vc[cell][row] (element (i, c) at c ldc + i); a workgroup
(row block b from vcol_lo, tile t) moves a 64 x 64 block through LDS, thread (wave w,
lane l) reading rows w, w + 4, ... at cell lane l and writing cells w, w + 4, ... at
row lane l. Every element of rows [lo, n0) of every cell < M is written exactly once,
with V's value, nothing else is touched and no access leaves either buffer -- for M
that is no multiple of 64 and a partial last row block.
CPU only: the device's own result is checked by tests/test_gpu_lattice_vcol.py
(test_store_content)."""
import numpy as np
import pytest

PBM, NT = 64, 256


def v_offset(tile, row, lane, vld):
    return tile * vld * PBM + row * PBM + lane


def vc_offset(tile, row, lane, ldc):
    return (tile * PBM + lane) * ldc + row


def build(V, Vc, lo, n0, M, vld, ldc):
    """k_vcol_build for one GP, workgroup by workgroup and thread by thread; returns the
    number of writes each element of Vc received."""
    tiles = (M + PBM - 1) // PBM
    hits = np.zeros(Vc.shape[0], dtype=np.int64)
    for b in range((n0 - lo + 63) // 64 if n0 > lo else 0):
        r0 = lo + 64 * b
        for tile in range(tiles):
            blk = np.full((64, 65), np.nan)
            for tid in range(NT):
                lane, w = tid & 63, tid >> 6
                for rr in range(w, 64, NT // 64):
                    if r0 + rr < n0:
                        o = v_offset(tile, r0 + rr, lane, vld)
                        assert 0 <= o < V.shape[0]
                        blk[rr, lane] = V[o]
            for tid in range(NT):
                lane, w = tid & 63, tid >> 6
                for cc in range(w, 64, NT // 64):
                    c = tile * PBM + cc
                    if c < M and r0 + lane < n0:
                        o = vc_offset(tile, r0 + lane, cc, ldc)
                        assert o == c * ldc + r0 + lane and 0 <= o < Vc.shape[0]
                        Vc[o] = blk[lane, cc]
                        hits[o] += 1
    return hits


@pytest.mark.parametrize("M", [1, 63, 64, 65, 130, 200])
@pytest.mark.parametrize("lo,n0", [(0, 1), (0, 64), (0, 65), (0, 127), (60, 70), (64, 200), (199, 200), (50, 50)])
def test_transposition_index_map(M, lo, n0):
    vld = ldc = 256                     # V's row capacity (a multiple of 128), shared by the store
    tiles = (M + PBM - 1) // PBM
    rng = np.random.default_rng(M * 1000 + n0)
    V = rng.standard_normal(tiles * vld * PBM)
    Vc = np.full(M * ldc, -7.0)         # the store is allocated for M cells, not for whole tiles
    hits = build(V, Vc, lo, n0, M, vld, ldc)
    want = np.zeros(M * ldc, dtype=np.int64)
    for c in range(M):
        want[c * ldc + lo:c * ldc + n0] = 1
    assert np.array_equal(hits, want)   # rows [lo, n0) of every cell once, nothing else
    for c in range(M):
        col = V[(c // PBM) * vld * PBM + np.arange(lo, n0) * PBM + c % PBM]
        assert np.array_equal(Vc[c * ldc + lo:c * ldc + n0], col)
        assert np.all(Vc[c * ldc:c * ldc + lo] == -7.0) and np.all(Vc[c * ldc + n0:(c + 1) * ldc] == -7.0)


def test_step_store_alignment_rule():
    """The cells' write-through of a step's k new rows (vcol_store): 16-byte stores cover
    elements [a, a + W) (W = 2 doubles or 4 floats) only where n0 leaves them aligned and
    all W rows are new; the rest go one by one. Every new row exactly once."""
    for W in (2, 4):
        for n0 in range(0, 9):
            for k in range(1, 17):
                KA = 8 if k <= 8 else 16
                seen = []
                al = n0 % W == 0
                for a in range(0, KA, W):
                    if al and a + W <= k:
                        assert (n0 + a) % W == 0
                        seen += list(range(a, a + W))
                    else:
                        seen += [a + b for b in range(W) if a + b < k]
                assert seen == list(range(k)), (W, n0, k)

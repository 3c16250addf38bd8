"""Which product lands in which element of the Delassus matrix: the circulant schedule of delassus_store (mocca_device.h) restated in numpy,
held against the tile-selection rule of the matrix-pipe build (delassus_tile_store).  No GPU: both are index arithmetic.

delassus_store, lane c (= dense column), step t = 0 .. nr // 2, rho = (c + t) mod nr, value v = J_rho . X_c:
    t == 0:  A[c][c] = 0, the product stays with lane c (the diagonal owner)
    t >= 1:  A[rho][c] = v   then   A[c][rho] = v          (two store instructions, all lanes at once, program order)
For even nr and t == nr / 2 two lanes write each of the two elements, and the later instruction wins: A[r][c] and A[c][r] then hold
different products.  The matrix-pipe build has every product D[r][c] = J_r . X_c in some lane and must send it to the same places.
"""
import numpy as np
import pytest

MAX_NR = 64


def store_schedule(nr):
    """-> (src, owner): src[i][j] = (r, c) of the product J_r . X_c that A[i][j] holds at the end (diagonal: None, stored as zero);
    owner[c] = (r, c) of the product lane c keeps as its diagonal."""
    src = [[None] * nr for _ in range(nr)]
    owner = [None] * nr
    for t in range(nr // 2 + 1):          # the steps are unrolled: step t of every lane comes before step t + 1 of any lane
        rho = [(c + t) % nr for c in range(nr)]
        if t == 0:
            for c in range(nr):
                assert rho[c] == c
                owner[c] = (rho[c], c)
                src[c][c] = None
            continue
        for c in range(nr):               # first store instruction of the step
            src[rho[c]][c] = (rho[c], c)
        for c in range(nr):               # second store instruction of the step
            src[c][rho[c]] = (rho[c], c)
    return src, owner


def tile_rule(nr):
    """The same two tables from delassus_tile_store: tile (R, C), lane l, register j holds D[r][c], r = 16 R + 4 (l >> 4) + j,
    c = 16 C + (l & 15); with e = (r - c) mod nr it is stored to A[c][r] when 2 e <= nr and to A[r][c] when 2 e < nr; the row's own
    lane then takes A[c][c] as its diagonal and stores the zero."""
    tiles = (nr + 15) // 16
    src = [[None] * nr for _ in range(nr)]
    writers = np.zeros((nr, nr), dtype=np.int64)
    for R in range(tiles):
        for C in range(tiles):
            for lane in range(64):
                li, lk = lane & 15, lane >> 4
                c = 16 * C + li
                for j in range(4):
                    r = 16 * R + 4 * lk + j
                    if not (r < nr and c < nr):
                        continue
                    e = r - c
                    if e < 0:
                        e += nr
                    if 2 * e <= nr:
                        src[c][r] = (r, c); writers[c][r] += 1
                    if 2 * e < nr and r != c:   # (the kernel stores the diagonal twice to the same address: one writer lane, one value)
                        src[r][c] = (r, c); writers[r][c] += 1
    owner = [src[c][c] for c in range(nr)]
    for c in range(nr):
        src[c][c] = None
    return src, owner, writers


@pytest.mark.parametrize("nr", range(1, MAX_NR + 1))
def test_tile_rule_names_the_products_of_the_store_schedule(nr):
    want, want_owner = store_schedule(nr)
    got, got_owner, writers = tile_rule(nr)
    assert got_owner == want_owner
    for i in range(nr):
        for j in range(nr):
            assert got[i][j] == want[i][j], (nr, i, j, got[i][j], want[i][j])
    assert (writers == 1).all()            # one writer per element: no store order to rely on


def test_even_row_counts_keep_both_orientations():
    """The case the rule exists for: at distance nr / 2 the two mirrored elements hold the two different products, each the transposed one."""
    for nr in range(2, MAX_NR + 1, 2):
        src, _ = store_schedule(nr)
        h = nr // 2
        for c in range(nr):
            r = (c + h) % nr
            assert src[r][c] == (c, r) and src[c][r] == (r, c)


def test_odd_row_counts_are_symmetric():
    for nr in range(1, MAX_NR + 1, 2):
        src, _ = store_schedule(nr)
        for i in range(nr):
            for j in range(nr):
                if i != j:
                    assert src[i][j] == src[j][i] and src[i][j] in ((i, j), (j, i))

"""Host restatement of k_vara_i8p's walk over the LOWER image of the digit slices (csrc/eagle_i8mfma.hip: VaraIt with `lower`, k_slice_w's
klive; no GPU).  Column tile ct of 256 W-columns runs the K stages of 128 W-rows [2 ct, max(klive, 2 ct + 2)): from its own diagonal block
down to the last live stage of W, never fewer than the two stages of the diagonal block.  Every (tile, stage) a worker -- or a piece
[pair0, pair1) of a cut last round -- must run is run exactly once, nothing beyond the padded size is touched, and the two tiles of a
pair (p, nct-1-p) cost the same whatever p wherever the floor does not bind, which is what keeps vara_tail_pieces and the work map of
tests/test_kernel_index_maps.py as they are."""
from test_kernel_index_maps import PMAX, vara_tail_pieces

SPT = 2  # T8 / BK8: K stages of 128 per column tile of 256


class It:
    """struct VaraIt + vit_set_tile + vit_advance, field for field."""

    def __init__(self, pair0, nct, npair, lower, klive):
        self.nct, self.npair, self.lower, self.klive = nct, npair, lower, klive
        self.p, self.half = pair0, 0
        self.set_tile()

    def set_tile(self):
        while self.p < self.npair:
            ct = self.p if self.half == 0 else self.nct - 1 - self.p
            if self.half == 1 and ct == self.p:
                self.p, self.half = self.p + 1, 0
                continue
            self.ct = ct
            self.kt = SPT * ct if self.lower else 0
            self.nk = SPT * (ct + 1)
            if self.lower and self.klive > self.nk:
                self.nk = self.klive
            self.valid = True
            return
        self.valid = False

    def advance(self):
        self.kt += 1
        if self.kt < self.nk:
            return
        if self.half == 0:
            self.half = 1
        else:
            self.half, self.p = 0, self.p + 1
        self.set_tile()


def walk(nct, klive, pair0, pair1, lower=True):
    """The kernel's main loop: per tile nk = it.nk - it.kt stages starting at the absolute stage it.kt (`nk >= 2` there)."""
    it = It(pair0, nct, pair1, lower, klive)
    out = []
    while it.valid:
        nk = it.nk - it.kt
        assert nk >= 2
        out += [(it.ct, it.kt + i) for i in range(nk)]
        it.kt = it.nk - 1
        it.advance()
    return out


def want(nct, klive, tiles):
    return sorted((ct, st) for ct in tiles for st in range(2 * ct, max(klive, 2 * ct + 2)))


def tiles_of(nct, pair0, pair1):
    return sorted({t for p in range(pair0, pair1) for t in (p, nct - 1 - p)})


def test_every_tile_and_stage_of_the_lower_walk_exactly_once():
    for nct in range(1, 42):
        npair = (nct + 1) // 2
        for klive in range(0, 2 * nct + 1):
            seen = walk(nct, klive, 0, npair)
            assert sorted(seen) == want(nct, klive, range(nct)), (nct, klive)
            assert len(set(seen)) == len(seen)
            assert all(st < 2 * nct for _, st in seen), (nct, klive)      # no stage at or beyond n_pad / 128
            assert all(st >= 2 * ct for ct, st in seen)


def test_pieces_of_a_cut_last_round_cover_their_pairs():
    for nct in range(1, 42):
        npair = (nct + 1) // 2
        for klive in (0, 1, nct, 2 * nct - 1, 2 * nct):
            for psplit in sorted({1, 2, min(npair, 3), min(npair, PMAX), vara_tail_pieces(5, npair)}):
                if psplit > npair:
                    continue
                allseen = []
                for piece in range(psplit):
                    pair0, pair1 = npair * piece // psplit, npair * (piece + 1) // psplit
                    seen = walk(nct, klive, pair0, pair1)
                    assert sorted(seen) == want(nct, klive, tiles_of(nct, pair0, pair1)), (nct, klive, psplit, piece)
                    allseen += seen
                assert sorted(allseen) == want(nct, klive, range(nct)), (nct, klive, psplit)


def test_pairs_cost_the_same_where_the_floor_does_not_bind():
    for nct in range(2, 42):
        for klive in range(0, 2 * nct + 1):
            for p in range(nct // 2):                                       # both tiles of the pair distinct
                cost = len(walk(nct, klive, p, p + 1))
                far = nct - 1 - p
                if klive >= 2 * far + 2:                                    # the floor binds on neither tile (the far one is the shorter)
                    assert cost == 2 * klive - 2 * (nct - 1), (nct, klive, p)
                else:
                    assert cost == max(klive - 2 * p, 2) + 2


def test_upper_walk_is_the_old_one():
    for nct in (1, 2, 5, 40):
        seen = walk(nct, 0, 0, (nct + 1) // 2, lower=False)
        assert sorted(seen) == sorted((ct, st) for ct in range(nct) for st in range(2 * (ct + 1)))


def test_headline_stage_count():
    """n = 10,000 -> n_pad = 10,240: 40 column tiles, 79 live stages of 80."""
    assert len(walk(40, 79, 0, 20)) == 1601
    assert len(walk(40, 80, 0, 20)) == len(walk(40, 0, 0, 20, lower=False)) == 1640
    assert len(walk(20, 40, 0, 10)) == 420                                  # n = 5,000 -> 5,120, pad 120: nothing dropped

"""The cases of tests/test_resource_edges_gpu.py against the C oracle.

The device tests expect what ``ctoken.first_collision`` says about hashlib's
map hashes.  Here the same cases, built by the same helpers, are run through
``ctoken.map_hashes`` and ``ctoken.first_collision`` and must give what their
construction intends: a break at the planted later part, or none.  So the
device tests' expectations rest on the construction and on the oracle, not on
one of them alone.
"""
import pytest

from oracle import ctoken
from tests_helpers import (EDGE_GUARDS, EDGE_LDS_GUARD_MAX, EDGE_PARTS, EDGE_SDU, EDGE_TILE, cut, edge_base,
                           edge_batched, edge_boundaries, edge_cases, edge_later_parts, edge_part, edge_single,
                           plant_repeats, sha_map_hashes)


def split4(hm):
    return [hm[i:i + 4] for i in range(0, len(hm), 4)]


def test_base_stream_has_no_repeat():
    stream, salt = edge_base()
    assert len(stream) == EDGE_PARTS * EDGE_SDU - 3 and len(salt) == 4
    hm = ctoken.map_hashes(stream, salt, EDGE_SDU)
    assert hm == sha_map_hashes(cut(stream), salt)
    assert len(set(split4(hm))) == EDGE_PARTS
    for guard in (1, 224, 100000):
        assert ctoken.first_collision(hm, guard) is None


def test_later_parts_sit_on_tile_edges():
    for guard in EDGE_GUARDS:
        cs = edge_later_parts(guard)
        lanes = {(c // EDGE_TILE > 0, c % EDGE_TILE) for c in cs}
        assert {(True, 0), (True, 1), (True, EDGE_TILE - 1)} <= lanes
        assert EDGE_PARTS - 1 in cs and EDGE_PARTS % EDGE_TILE != 0
        assert ((EDGE_TILE - 1) in cs) == (guard < EDGE_TILE - 1)
        assert all(c > guard for c in cs)


@pytest.mark.parametrize("guard", EDGE_GUARDS)
def test_window_edges_single(guard):
    """Distance guard breaks at c, distance guard + 1 is accepted."""
    for a, c, expect in edge_cases(guard):
        stream, salt, hm, col = edge_single(guard, a, c)
        assert hm == ctoken.map_hashes(stream, salt, EDGE_SDU)
        assert len(hm) == 4 * EDGE_PARTS and hm[4 * a:4 * a + 4] == hm[4 * c:4 * c + 4]
        assert col == expect, (a, c)
        assert c - a == (guard if expect is not None else guard + 1)


@pytest.mark.parametrize("guard", EDGE_GUARDS)
def test_window_edges_batched(guard):
    lay, cases = edge_batched(guard)
    assert lay.n_parts % EDGE_TILE == 101 and cases[-1][1] == lay.n_parts - 1
    assert sorted(c % EDGE_TILE for _, c, _ in cases) == [0, 0, 1, 1, 100, 100, EDGE_TILE - 1, EDGE_TILE - 1]
    hit_res = {r: c for r, c, hit in cases if hit}
    for r in range(lay.n_res):
        assert lay.first[r] == hit_res.get(r, -1), r
    for r, c, hit in cases:
        assert c >= EDGE_TILE and lay.res[c] == r and lay.start[r] == c - guard - 1
        hm = ctoken.map_hashes(lay.data[lay.off[lay.start[r]]:lay.off[c] + lay.len[c]], lay.salts[r], EDGE_SDU)
        assert ctoken.first_collision(hm, guard) == (guard + 1 if hit else None)
        assert hm == lay.hashes[r][:len(hm)]
        if guard <= EDGE_LDS_GUARD_MAX:           # the LDS kernel takes its mixed path for this tile
            assert lay.mixed_window(c)


def test_guard_larger_than_resource():
    stream = plant_repeats(edge_base()[0][:300 * EDGE_SDU], [(0, 299)])
    hm = ctoken.map_hashes(stream, edge_base()[1], EDGE_SDU)
    for guard in (4096, 100000):
        assert ctoken.first_collision(hm, guard) == 299
    assert ctoken.first_collision(hm, 298) is None


def test_earliest_of_several():
    from tests_helpers import SEVERAL, several_two_resources
    stream, salt = edge_base()
    hm = ctoken.map_hashes(plant_repeats(stream, SEVERAL), salt, EDGE_SDU)
    assert len({c // EDGE_TILE for _, c in SEVERAL}) == 3 and all(c - a <= 224 for a, c in SEVERAL)
    for guard in (224, 4097):
        assert ctoken.first_collision(hm, guard) == min(c for _, c in SEVERAL)
        lay = several_two_resources(guard)
        assert lay.first == [2600, 3000 + 2950]
        assert lay.first[1] // EDGE_TILE == (lay.n_parts - 1) // EDGE_TILE      # the launch's last tile


@pytest.mark.parametrize("guard", [224, 600])
def test_resource_boundaries(guard):
    lay, nm = edge_boundaries(guard)
    half = guard // 2 + 1
    A, B, C, D, E, F = (nm[k] for k in "ABCDEF")
    assert lay.start[B] % EDGE_TILE != 0 and lay.start[D] % EDGE_TILE == 0 and lay.start[F] % EDGE_TILE != 0
    for x, y in ((A, B), (C, D)):                 # equal hashes on both sides, inside the window
        assert lay.hashes[y][:4 * half] == lay.hashes[x][-4 * half:] and half <= guard
        assert lay.first[x] == -1 and lay.first[y] == -1
    assert len({lay.hashes[r] for r in nm["ones"]}) == 1 and all(lay.first[r] == -1 for r in nm["ones"])
    assert lay.hashes[F][:4] == lay.hashes[E][-4:] == lay.hashes[F][4 * guard:4 * guard + 4]
    assert lay.first[E] == -1 and lay.first[F] == lay.start[F] + guard
    if guard == 600:                              # the window of B's last copy holds the boundary and spans three tiles
        j = lay.start[B] + half - 1
        assert j - guard < lay.start[B] and j // EDGE_TILE - (j - guard) // EDGE_TILE + 1 == 3
    # the whole launch as one resource would collide at B's first part: the boundaries are what prevents it
    assert ctoken.first_collision(b"".join(lay.hashes), guard) == lay.start[B]
    assert edge_part(0) == lay.parts[0]

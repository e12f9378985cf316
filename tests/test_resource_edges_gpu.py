"""Resource hashmap kernels (resource_kernels.hip) at window, tile and tail edges.

``k_map_collisions_lds`` (guards up to 4096) and ``k_map_collisions`` (larger
guards) against ``ctoken.first_collision`` over hashlib's map hashes, with a
repeat planted on the oldest place of the window and one place past it, for
later parts on the first, second and last lane of a tile >= 1, in the partial
last tile and in tile 0; several repeats per resource; equal hashes on both
sides of resource boundaries.  ``k_map_hashes`` on both sides of every
block-count step of its tail for salts of 0 to 130 bytes, at every byte phase
of a part's start and at launch sizes around a workgroup.  All bit-exact.
tests/test_resource_edges.py ties the same cases to the C oracle.
"""
import numpy as np
import pytest

import reticulum_amd as rt
from tests_helpers import (EDGE_GUARDS, EDGE_SDU, SEVERAL, Layout, cut, edge_base, edge_batched, edge_boundaries,
                           edge_cases, edge_single, plant_repeats, several_two_resources, sha_map_hashes)

pytestmark = pytest.mark.gpu

PAD = 64                      # guard bytes behind the map hashes
FC_PAD, FC_JUNK = 4, 0x5A5A5A5A


def launch(data, salts, n_parts, off=None, ln=None, res=None, sdu=EDGE_SDU, guard=0, want_fc=True):
    """``device.map_hashes`` over host inputs: (map hashes, first_collision as
    an int32 array or None).  Both outputs start out as junk and have guard
    words behind them, which must come back untouched."""
    import torch
    from reticulum_amd import device
    S = len(salts[0])
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    s = torch.from_numpy(np.frombuffer(b"".join(salts), np.uint8).reshape(len(salts), S).copy()).cuda()
    out = torch.full((4 * n_parts + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    fc = torch.full((len(salts) + FC_PAD,), FC_JUNK, dtype=torch.int32, device="cuda") if want_fc else None
    t = lambda a, dt: None if a is None else torch.tensor(np.asarray(a), dtype=dt).cuda()
    device.map_hashes(d, out[:4 * n_parts], s, t(off, torch.int64), t(ln, torch.int32), t(res, torch.int32), sdu=sdu,
                      guard=guard, first_collision=None if fc is None else fc[:len(salts)])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[4 * n_parts:] == 0xA5).all(), "wrote behind the map hashes"
    if fc is None:
        return got[:4 * n_parts].tobytes(), None
    fch = fc.cpu().numpy()
    assert (fch[len(salts):] == FC_JUNK).all(), "wrote behind first_collision"
    return got[:4 * n_parts].tobytes(), fch[:len(salts)]


def launch_layout(lay, guard=None, want_fc=True):
    return launch(lay.data, lay.salts, lay.n_parts, lay.off, lay.len, lay.res,
                  guard=lay.guard if guard is None else guard, want_fc=want_fc)


def three_forms(stream, salt, guard):
    """(form, map hashes, first collision or None) of one resource of 8-byte
    parts through the host call (part_res null), the device call with explicit
    parts all of resource 0, and the uniform device call."""
    n = -(-len(stream) // EDGE_SDU)
    yield ("host",) + rt.resource_hashmap(stream, salt, sdu=EDGE_SDU, guard=guard)
    off = [EDGE_SDU * j for j in range(n)]
    ln = [min(EDGE_SDU, len(stream) - o) for o in off]
    for form, parts in (("explicit", (off, ln, [0] * n)), ("uniform", ())):
        hm, fc = launch(stream, [salt], n, *parts, guard=guard)
        yield form, hm, (None if fc[0] == -1 else int(fc[0]))


@pytest.mark.parametrize("guard", EDGE_GUARDS)
def test_window_edges_single(guard):
    """One resource of 6000 parts (the LDS kernel's one-resource path for
    guards up to 4096, k_map_collisions above): a copy at distance guard
    breaks at the later part, a copy at distance guard + 1 is accepted."""
    for a, c, _ in edge_cases(guard):
        stream, salt, hm, col = edge_single(guard, a, c)
        for form, got_hm, got_col in three_forms(stream, salt, guard):
            assert got_hm == hm, (form, a, c)
            assert got_col == col, (form, a, c)


@pytest.mark.parametrize("guard", EDGE_GUARDS)
def test_window_edges_batched(guard):
    """The same edges with every case a resource of its own in one launch, so
    that the LDS kernel's tile holds a resource boundary (its mixed path);
    first_collision holds global part indices."""
    lay, cases = edge_batched(guard)
    hm, fc = launch_layout(lay)
    assert hm == b"".join(lay.hashes)
    for r, c, hit in cases:
        assert fc[r] == (c if hit else -1), (r, c, hit)
    assert fc.tolist() == lay.first


@pytest.mark.parametrize("guard", [4096, 100000])
def test_guard_larger_than_resource(guard):
    stream, salt = edge_base()
    stream = plant_repeats(stream[:300 * EDGE_SDU], [(0, 299)])
    hm = sha_map_hashes(cut(stream), salt)
    for form, got_hm, got_col in three_forms(stream, salt, guard):
        assert got_hm == hm and got_col == 299, form


@pytest.mark.parametrize("guard", [224, 4097])
def test_earliest_of_several(guard):
    """Three repeats in three tiles of one resource: the smallest later part
    wins; two resources in one launch keep their minima apart."""
    from oracle import ctoken
    stream, salt = edge_base()
    stream = plant_repeats(stream, SEVERAL)
    hm = sha_map_hashes(cut(stream), salt)
    col = ctoken.first_collision(hm, guard)
    for form, got_hm, got_col in three_forms(stream, salt, guard):
        assert got_hm == hm and got_col == col == 5400, form
    lay = several_two_resources(guard)
    hm2, fc = launch_layout(lay)
    assert hm2 == b"".join(lay.hashes) and fc.tolist() == lay.first == [2600, 5950]


@pytest.mark.parametrize("guard", [224, 600])
def test_resource_boundaries(guard):
    """Equal map hashes on the other side of a resource boundary, inside the
    window, are no collision; a repeat reaching back to the resource's own
    first part is one."""
    lay, nm = edge_boundaries(guard)
    hm, fc = launch_layout(lay)
    assert hm == b"".join(lay.hashes)
    for k in "ABCDE":
        assert fc[nm[k]] == -1, k
    assert (fc[nm["ones"].start:nm["ones"].stop] == -1).all()
    assert fc[nm["F"]] == lay.start[nm["F"]] + guard
    assert fc.tolist() == lay.first


def random_parts(rng, lengths):
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lengths]


@pytest.mark.parametrize("salt_len", [0, 1, 4, 32, 55, 56, 60, 63, 64, 119, 120, 130])
def test_tail_blocks(salt_len):
    """Parts of every length 0..200 in neighbouring lanes, for two resources
    with salts of their own.  The tail is (rem + salt_len + 8) / 64 + 1 blocks
    and rem runs through 0..63 three times, so for every salt length the step
    it can reach (1 to 2 blocks at rem + salt_len = 56, 2 to 3 at 120, 3 to 4
    at 184) falls between neighbouring lanes; length 0 is get_map_hash(b"")."""
    rng = np.random.Generator(np.random.PCG64(7200 + salt_len))
    salts = random_parts(rng, [salt_len, salt_len])
    lay = Layout([random_parts(rng, range(201)), random_parts(rng, range(201))], salts, 0)
    assert {(n % 64 + salt_len + 8) // 64 for n in lay.len} >= {(salt_len + 8) // 64, (salt_len + 71) // 64}
    hm, _ = launch_layout(lay, want_fc=False)
    exp = b"".join(lay.hashes)
    bad = [(lay.res[j], lay.len[j]) for j in range(lay.n_parts) if hm[4 * j:4 * j + 4] != exp[4 * j:4 * j + 4]]
    assert not bad, bad[:8]


@pytest.mark.parametrize("salt_len", [4, 32])
def test_tail_phases(salt_len):
    """Parts with full blocks starting at every byte phase of a 16-byte line."""
    rng = np.random.Generator(np.random.PCG64(7300 + salt_len))
    salt = random_parts(rng, [salt_len])[0]
    data = rng.integers(0, 256, 80 * 480, dtype=np.uint8).tobytes()
    off, ln = [], []
    for L in (64, 65, 127, 128, 464):
        for phase in range(16):
            off.append(480 * len(off) + phase)
            ln.append(L)
    hm, _ = launch(data, [salt], len(off), off, ln, want_fc=False)
    exp = sha_map_hashes([data[o:o + n] for o, n in zip(off, ln)], salt)
    bad = [(ln[j], off[j] % 16) for j in range(len(off)) if hm[4 * j:4 * j + 4] != exp[4 * j:4 * j + 4]]
    assert not bad, bad[:8]


@pytest.mark.parametrize("sdu", [1, 63, 64, 65, 464])
def test_launch_sizes(sdu):
    """The uniform form at 1, 255, 256 and 257 parts with a short last part:
    the last lane of a workgroup, and one lane alone in the next."""
    from oracle import ctoken
    rng = np.random.Generator(np.random.PCG64(7400 + sdu))
    salt = random_parts(rng, [4])[0]
    for n in (1, 255, 256, 257):
        data = random_parts(rng, [(n - 1) * sdu + max(1, sdu // 2)])[0]
        exp = sha_map_hashes(cut(data, sdu), salt)
        assert len(exp) == 4 * n
        hm, fc = launch(data, [salt], n, sdu=sdu, guard=224)
        assert hm[-4:] == exp[-4:] and hm == exp, n
        col = ctoken.first_collision(exp, 224)
        assert fc[0] == (-1 if col is None else col), n
        assert rt.resource_hashmap(data, salt, sdu=sdu) == (exp, col), n


def test_no_collision_output():
    """Without first_collision the launch writes the map hashes and nothing
    behind them, whatever the guard."""
    a, c, _ = edge_cases(224)[0]
    stream, salt, hm, col = edge_single(224, a, c)
    assert col == c
    n = len(hm) // 4
    for guard in (224, 4097):
        assert launch(stream, [salt], n, guard=guard, want_fc=False) == (hm, None)
    lay = several_two_resources(224)
    assert launch_layout(lay, want_fc=False) == (b"".join(lay.hashes), None)


def test_guard_zero_reports_none():
    """guard = 0 compares nothing: every entry of first_collision is -1, also
    for resources that repeat parts."""
    lay = several_two_resources(224)
    hm, fc = launch_layout(lay, guard=0)
    assert hm == b"".join(lay.hashes) and fc.tolist() == [-1, -1]
    a, c, _ = edge_cases(224)[0]
    stream, salt, hm1, _ = edge_single(224, a, c)
    got, fc = launch(stream, [salt], len(hm1) // 4, guard=0)
    assert got == hm1 and fc.tolist() == [-1]

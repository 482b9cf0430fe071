"""GPU: the prefix cache's digest launch on its own (page_digest_kernel through sv_debug_page_digests) against the numpy restatement in
tests/prefix_key_ref.py, bit for bit: ragged and rectangular forms, independence of the packed offset and of the neighbours, and that one bit
or one swap of rows changes exactly the digest of the page it lies in."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import starvector_oracle as O
from starvector_amd import _lib
from tests import prefix_key_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

LENS = [64, 65, 127, 128, 130, 259]
HIDDENS = [O.OracleConfig.tiny().hidden, 2048]


def _rows(lens, hidden, seed):
    """uint16 bit patterns: every bf16 pattern may occur (the digest is over bits, not values)"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << 16, size=(n, hidden), dtype=np.uint16) for n in lens]


def _digests(seqs, hidden, lens=None, S0=0):
    """the launch over `seqs` packed back to back -> per prompt the list of its full pages' (a, b)"""
    lib = _lib.load()
    packed = torch.from_numpy(np.concatenate(seqs).astype(np.int16)).to(dev()).contiguous()
    n = len(seqs)
    max_pages = max(max(s.shape[0] // 64 for s in seqs), 1) + 1       # one entry more than anyone needs: it must stay zero
    out = (C.c_uint64 * (n * max_pages * 2))()
    arr = (C.c_int32 * n)(*lens) if lens is not None else None
    rc = lib.sv_debug_page_digests(C.c_void_p(packed.data_ptr()), n, arr, S0, hidden, max_pages, out, None)
    assert rc == 0, lib.sv_last_error().decode()
    res = []
    for u, s in enumerate(seqs):
        full = s.shape[0] // 64
        row = [(out[2 * (u * max_pages + k)], out[2 * (u * max_pages + k) + 1]) for k in range(max_pages)]
        assert all(d == (0, 0) for d in row[full:]), "an entry beyond the full pages was written"
        res.append(row[:full])
    return res


@pytest.fixture(scope="module", params=HIDDENS)
def case(request):
    hidden = request.param
    seqs = _rows(LENS, hidden, 100 + hidden)
    return hidden, seqs, [R.prompt_digests(s) for s in seqs], _digests(seqs, hidden, LENS)


def test_digests_are_the_restatement_bit_for_bit(case):
    hidden, seqs, ref, got = case
    assert [len(g) for g in got] == [n // 64 for n in LENS]
    assert got == ref
    flat = [d for g in got for d in g]
    assert len(set(flat)) == len(flat)                            # different pages, different digests


def test_offset_and_neighbours_do_not_enter(case):
    hidden, seqs, ref, got = case
    other = _rows([33, 70], hidden, 7)
    moved = _digests([other[0], seqs[5], other[1], seqs[3]], hidden, [33, 259, 70, 128])
    assert moved[1] == got[5] and moved[3] == got[3] and moved[0] == []
    assert moved[2] == R.prompt_digests(other[1])


def test_one_bit_and_one_swap_change_exactly_their_page(case):
    hidden, seqs, ref, got = case
    flipped = [s.copy() for s in seqs]
    flipped[5][63, hidden - 1] ^= 1                              # the last element of row 63 of the 259-row prompt: page 0
    g = _digests(flipped, hidden, LENS)
    assert g[5][0] != got[5][0] and g[5][0][0] != got[5][0][0] and g[5][0][1] != got[5][0][1]
    assert g[5][1:] == got[5][1:] and g[:5] == got[:5]
    assert g[5][0] == R.page_digest(flipped[5][:64])
    swapped = [s.copy() for s in seqs]
    swapped[4][[0, 1]] = swapped[4][[1, 0]]                      # rows 0 and 1 of the 130-row prompt
    g = _digests(swapped, hidden, LENS)
    assert g[4][0] != got[4][0] and g[4][1:] == got[4][1:] and g[:4] == got[:4] and g[5] == got[5]
    assert g[4][0] == R.page_digest(swapped[4][:64])
    swapped = [s.copy() for s in seqs]
    swapped[0][10, [4, 5]] = swapped[0][10, [5, 4]]              # two elements of one 64-bit word
    g = _digests(swapped, hidden, LENS)
    assert g[0][0] != got[0][0] and g[1:] == got[1:]


def test_the_rectangular_form_equals_the_ragged_form(case):
    hidden = case[0]
    for S0 in (64, 130):
        seqs = _rows([S0] * 3, hidden, S0)
        rag = _digests(seqs, hidden, [S0] * 3)
        assert _digests(seqs, hidden, None, S0) == rag == [R.prompt_digests(s) for s in seqs]

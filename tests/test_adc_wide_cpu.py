"""CPU: the workspace and the argument checks of mivq_adc_search on the shapes whose lookup tables
do not fit one workgroup's LDS (M * 2^nbits * 4 B > 160 KiB), all answered before any HIP call."""

import ctypes

import pytest

WIDE = [(192, 8), (161, 8), (768, 6), (2600, 4)]


@pytest.fixture(scope="module")
def lib():
    from haag_vq import _native

    return _native.load_library()


@pytest.mark.parametrize("M,nbits", WIDE)
def test_wide_shapes_have_a_workspace(lib, M, nbits):
    assert lib.mivq_adc_search_workspace_bytes(100, 10_000, M, nbits, 10) > 0
    assert lib.mivq_adc_search_workspace_bytes(100, 10_000, M, 9, 10) == 0
    assert lib.mivq_adc_search_workspace_bytes(100, 10_000, M, nbits, 0) == 0


def test_resident_table_shapes_keep_their_workspace(lib):
    """M = 128 / 160 at 8 bits stay on the resident-table scan: the sizes of the commit before the
    wide scan (1 row chunk x 16 part lists x 100 queries x 10 x 8 B)."""
    assert lib.mivq_adc_search_workspace_bytes(100, 10_000, 128, 8, 10) == 640_000
    assert lib.mivq_adc_search_workspace_bytes(100, 10_000, 160, 8, 10) == 640_000


def test_wide_workspace_is_part_lists_only(lib):
    """1000 queries x 1M rows: the wide scan cuts the rows into 2 ranges of 16 part lists (125 query
    blocks x 2 fill 256 CUs once), the resident-table scan of M = 16, k = 33 (no filtered path) into
    2 chunks of 16.  Equal part counts, so the constant is 1: the wide workspace (k = 10) must not
    exceed the other (k = 33), which a term in n * nq (4 GB) or in M would."""
    wide = lib.mivq_adc_search_workspace_bytes(1000, 1_000_000, 768, 8, 10)
    narrow = lib.mivq_adc_search_workspace_bytes(1000, 1_000_000, 16, 8, 33)
    assert 0 < wide <= 1 * narrow, (wide, narrow)


def test_wide_argument_checks(lib):
    from haag_vq import _native

    p, nq, n, M, k = ctypes.c_void_p(0x10000), 3, 5000, 192, 10
    need = lib.mivq_adc_search_workspace_bytes(nq, n, M, 8, k)

    def call(k=k, ws=p, nb=need, flags=0):
        return lib.mivq_adc_search(p, nq, p, n, M, 8, k, 0, ws, nb, p, p, flags, None)

    assert call(nb=need - 1) == _native.MIVQ_ERR_WORKSPACE
    assert call(ws=None) == _native.MIVQ_ERR_WORKSPACE
    assert call(k=257) == _native.MIVQ_ERR_UNSUPPORTED
    assert call(flags=8) == _native.MIVQ_ERR_INVALID

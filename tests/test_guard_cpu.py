"""The guard-band arena checks itself on CPU tensors, the case tables of the bounds tests cover
every entry point of the C ABI, and every entry point with a workspace refuses a short or null
one on the host, before any launch."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _bounds as B  # noqa: E402
import _guard as G  # noqa: E402

CPU = torch.device("cpu")
SIZE = 4 * G.GUARD + G.TAIL + 8192


# ------------------------------------------------------------------------------ the arena
def test_clean_arena_reports_nothing():
    a = G.Arena(CPU, SIZE)
    x = a.carve("x", 100)
    y = a.carve("y", 0)
    assert x.numel() == 100 and y.numel() == 0 and (x == G.POISON).all()
    x.fill_(7)  # a buffer's own bytes are its own
    assert a.violations() == []
    a.assert_clean("clean")


def test_one_byte_past_a_carve_is_reported():
    a = G.Arena(CPU, SIZE)
    x = a.carve("x", 100, fill=0)
    a.buf[a.carves[0].start + 100] = 0
    assert a.violations() == [("x", "after", 0, 1)]
    with pytest.raises(AssertionError, match=r"after buffer 'x', nearest 0 B"):
        a.assert_clean("case")
    assert (x == 0).all()


def test_one_byte_before_a_carve_is_reported():
    a = G.Arena(CPU, SIZE)
    a.carve("x", 100)
    a.buf[a.carves[0].start - 1] = 0
    assert a.violations() == [("x", "before", 0, 1)]


def test_last_guard_byte_is_reported():
    a = G.Arena(CPU, SIZE)
    a.carve("x", 100)
    s = a.carves[0].start
    a.buf[s + 100 + G.GUARD - 1] = 1
    a.buf[s - G.GUARD] = 1
    assert a.violations() == [("x", "before", G.GUARD - 1, 1), ("x", "after", G.GUARD - 1, 1)]


def test_a_store_past_every_guard_is_reported():
    a = G.Arena(CPU, SIZE)
    a.carve("x", 100)
    a.buf[-1] = 0
    (name, side, _, count), = a.violations()
    assert (name, side, count) == ("<tail>", "after", 1)


def test_guards_of_neighbours_are_told_apart():
    a = G.Arena(CPU, SIZE + 2 * G.GUARD)
    a.carve("x", 64)
    a.carve("y", 64)
    a.buf[a.carves[1].start - 3: a.carves[1].start] = 0
    assert a.violations() == [("y", "before", 0, 3)]


@pytest.mark.parametrize("align,skew", [(256, 0), (256, 4), (16, 1), (4096, 8), (1, 0)])
def test_align_and_skew_are_honoured(align, skew):
    a = G.Arena(CPU, SIZE + 2 * G.GUARD + 8192)
    a.carve("first", 13)
    v = a.carve("x", 40, align=align, skew=skew)
    assert (v.data_ptr() - skew) % align == 0
    assert a.ptr("x").value == v.data_ptr()
    c = a.carves[1]
    assert c.start - (a.carves[0].start + 13) >= 2 * G.GUARD  # both guards whole
    assert a.violations() == []


def test_fill_and_typed_views():
    a = G.Arena(CPU, SIZE)
    src = np.arange(6, dtype=np.float32)
    v = a.carve("x", 24, fill=src)
    np.testing.assert_array_equal(G.typed(v, "float32").numpy(), src)
    np.testing.assert_array_equal(G.typed(v, "int32", (2, 3)).numpy(), src.view(np.int32).reshape(2, 3))
    assert G.ptr(v).value == v.data_ptr() and G.ptr(None) is None
    np.testing.assert_array_equal(G.to_numpy(v), src.view(np.uint8))
    with pytest.raises(ValueError, match="fill has"):
        a.carve("y", 8, fill=src)
    w = a.carve("z", 5, fill=0xFF)
    assert (w == 0xFF).all() and a.violations() == []


def test_a_carve_that_eats_the_tail_is_refused():
    a = G.Arena(CPU, SIZE)
    with pytest.raises(ValueError, match="would leave less than"):
        a.carve("big", 2 * G.GUARD + 8192 + 1)
    a.carve("ok", 4096)
    with pytest.raises(ValueError, match="name already used"):
        a.carve("ok", 16)
    assert G.arena_bytes([100, 0, 4096]) >= 100 + 4096 + 6 * G.GUARD + G.TAIL
    b = G.Arena(CPU, G.arena_bytes([100, 0, 4096]))
    for i, n in enumerate([100, 0, 4096]):
        b.carve(str(i), n, skew=4)


# ------------------------------------------------------------------------------ coverage
SIZE_QUERY = "a size query: takes no pointer, checked by the refusal test and used by every case with a workspace"
EXCLUDED = {
    "mivq_last_error": "returns the thread's error string, takes no buffer",
    "mivq_abi_version": "returns a constant",
    "mivq_device_info": "fills host variables of the caller, no device pointer",
    "mivq_pq_prep_bytes": "a size query: sizes the prep buffer of every mivq_pq_prepare case",
    "mivq_opq_prep_bytes": "a size query: sizes the prep buffer of every mivq_opq_prepare case",
}
# entry points with no empty call to make
NO_EMPTY = {
    "mivq_pq_prepare": "takes a codebook, no row count",
    "mivq_opq_prepare": "takes a matrix, no row count",
    "mivq_column_mean": "documented for n >= 1 only (the mean of no rows)",
}


def _signatures():
    from haag_vq import _native

    return _native.SIGNATURES


def _workspace_queries():
    return sorted(n for n in _signatures() if n.endswith("_workspace_bytes"))


def _entry_of(query: str) -> str:
    special = {"mivq_opq_rotate_workspace_bytes": "mivq_opq_rotate_prepared",
               "mivq_codebook1d_workspace_bytes": "mivq_codebook1d_fit"}
    return special.get(query, query[:-len("_workspace_bytes")])


def test_every_entry_point_has_a_case_or_a_reason():
    sig = _signatures()
    covered = {c.entry for c in B.all_cases()}
    excluded = dict(EXCLUDED, **{q: SIZE_QUERY for q in _workspace_queries()})
    assert not covered & set(excluded), sorted(covered & set(excluded))
    missing = sorted(set(sig) - covered - set(excluded))
    assert not missing, f"entry points with no buffer-contract case (tests/_bounds_*.py) and no exclusion: {missing}"
    stale = sorted((covered | set(excluded)) - set(sig))
    assert not stale, f"cases or exclusions for names that are not in SIGNATURES: {stale}"
    assert all(len(r) > 10 for r in list(excluded.values()) + list(NO_EMPTY.values()))


def test_every_entry_point_has_a_ragged_an_edge_and_an_empty_case():
    by_entry = {}
    for c in B.all_cases():
        assert c.tags <= {B.RAGGED, B.EDGE, B.EMPTY} and c.tags, c
        by_entry.setdefault(c.entry, set()).update(c.tags)
    for entry, tags in sorted(by_entry.items()):
        want = {B.RAGGED, B.EDGE} | (set() if entry in NO_EMPTY else {B.EMPTY})
        assert want <= tags, f"{entry}: no {sorted(want - tags)} case"
    assert set(NO_EMPTY) <= set(by_entry)


def test_case_builders_run_without_a_gpu(oracle):
    """Every builder gives an argument list that matches the entry's signature, buffers with
    distinct names, and at most one workspace."""
    sig = _signatures()
    for c in B.all_cases():
        call = c.build(oracle)
        nargs = sum(2 if isinstance(a, B.Ws) else 1 for a in call.args)
        assert nargs == len(sig[c.entry][1]), (c, nargs, len(sig[c.entry][1]))
        names = [b.name for b in call.bufs()]
        assert len(set(names)) == len(names) and "workspace" not in names, c
        assert (call.ws() is not None) == (c.entry in {_entry_of(q) for q in _workspace_queries()}), c
        assert B.EMPTY in c.tags or call.expect is not None, c


# ------------------------------------------------------------------------------ workspace refusal
@pytest.mark.parametrize("query", [
    "mivq_adc_search_workspace_bytes", "mivq_bucket_sort_workspace_bytes", "mivq_codebook1d_workspace_bytes",
    "mivq_extrabitq_flat_search_workspace_bytes", "mivq_flat_search_workspace_bytes",
    "mivq_ivf_listpq_search_workspace_bytes", "mivq_ivf_lvq_search_workspace_bytes",
    "mivq_ivf_rabitq_search_workspace_bytes", "mivq_ivf_sq_search_workspace_bytes", "mivq_ivfpq_search_workspace_bytes",
    "mivq_lvq_flat_search_workspace_bytes", "mivq_opq_gram_workspace_bytes", "mivq_opq_rotate_workspace_bytes",
    "mivq_pq_encode_workspace_bytes", "mivq_rabitq_flat_search_workspace_bytes", "mivq_rabitq_search_workspace_bytes",
    "mivq_rankaware_flat_search_workspace_bytes", "mivq_rerank_f32_workspace_bytes", "mivq_rerank_lvq2_workspace_bytes",
    "mivq_rerank_lvq_workspace_bytes", "mivq_rerank_sq_workspace_bytes", "mivq_sq_flat_search_workspace_bytes",
])
def test_short_and_null_workspaces_are_refused_on_the_host(oracle, query):
    """At the entry's first ragged case: need - 1 bytes, and a null workspace of `need` bytes, both
    return MIVQ_ERR_WORKSPACE.  Every device pointer is a fake address: nothing is launched."""
    from haag_vq import _native

    lib = _native.load_library()
    assert query in _workspace_queries()
    entry = _entry_of(query)
    case = next(c for c in B.all_cases() if c.entry == entry and B.RAGGED in c.tags)
    assert case.build(oracle).ws().query == query
    need, short, null = B.refusal_codes(case, oracle, lib)
    assert need > 0, (case, need)
    assert short == B.ERR_WORKSPACE, f"{case}: {need - 1} of {need} bytes returned {short}"
    assert null == B.ERR_WORKSPACE, f"{case}: a null workspace of {need} bytes returned {null}"


def test_the_refusal_list_is_the_list_of_queries():
    marks = [m for m in test_short_and_null_workspaces_are_refused_on_the_host.pytestmark if m.name == "parametrize"]
    assert sorted(marks[0].args[1]) == _workspace_queries()

"""The buffer contract of include/mivq.h, entry point by entry point: the searches, the re-ranking
entries, the top-k / IVF building blocks and the IVF searches.

The properties P1 .. P5 are those of tests/test_bounds_codec_gpu.py; the cases are in
tests/_bounds_search.py.  An empty search is nq = 0 and n = 0; mivq_topk_merge at parts = 0,
mivq_bucket_sort and mivq_ivf_sq_fit at n = 0 are checked against what the header documents for
them (the sentinel lists, zero offsets, the parameters of empty lists).  Every P4 reference is a
rule module or the oracle: the flat searches over codes against oracle.flat_search on the rule's
decode, the IVF searches against the `expected` of their rule modules, bit for bit; the rows of
mivq_ivf_rabitq_encode as in test_rabitq_parity (factors within 1e-5).

Branches left out for size: a second chunk of queries in mivq_ivf_listpq_search (its host
reference composes 266k oracle calls at the shape that needs one; test_ivf_listpq_gpu.py covers it
through the wrapper), and ids or offsets past 2^31 rows.
"""

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _bounds as B  # noqa: E402
import _bounds_search  # noqa: E402,F401

CASES = [c for c in B.CASES if c.build.__module__ == "_bounds_search"]


@pytest.mark.parametrize("case", CASES, ids=[f"{c.entry[5:]}-{c.id}" for c in CASES])
def test_buffer_contract(dev, oracle, case):
    B.run_case(case, dev, oracle)

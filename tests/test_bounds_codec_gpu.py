"""The buffer contract of include/mivq.h, entry point by entry point: the codecs.

Every case (tests/_bounds_codec.py) calls the raw C entry point with every pointer carved from
one guard-banded arena (tests/_guard.py): outputs of exactly their documented size, the workspace
of exactly *_workspace_bytes() bytes, inputs at the alignment the case names.  Checked per case:

  P1  no stray write: every guard band and the arena's tail still hold their poison;
  P2  inputs are read-only: byte-identical after the call;
  P3  the result does not depend on what the workspace and the pure outputs held before: the call
      runs twice, over 0x00 and over 0xFF (NaN as a float, -1 as an int32, the largest uint32), and
      every output is byte-identical, which also shows that every output byte is written; in/out
      buffers (the centroids and counts of mivq_kmeans_update) get the same data both times;
  P4  the outputs equal the reference, under the comparison the entry point's own test uses (bit
      for bit except the two factors of a RaBitQ-1 code row, 1e-5 as in test_rabitq_parity);
  P5  an empty call (n = 0) returns MIVQ_OK and leaves poisoned outputs untouched, but for what
      the header documents: zero counts (kmeans_update), a zero Gram matrix.

References are the rule modules and the oracle.  Entry points whose P4 reference is the plain
_native wrapper on the same inputs, for want of an importable bit-exact one: mivq_pq_prepare and
mivq_opq_prepare (the derived images), mivq_extrabitq_normalize and mivq_extrabitq_quantize (the
rule module bounds their norms and t instead of restating the device's summation order).
mivq_opq_rotate, mivq_opq_rotate_prepared, mivq_opq_gram, mivq_extrabitq_rotate and
mivq_kmeans_update run on small integers, where every sum is exact in any order and numpy's
integer product is the reference.

Branches left out for size: the wide PQ filters (dsub >= 128, thousands of rows per workgroup) and
the 2^20-row slicing of mivq_pq_encode; the pair table of mivq_pq_prepare above 64 subspaces; d
above 2^14 in mivq_extrabitq_rotate's 32-bit offset switch.  test_kernels_gpu.py and
test_pq_scale_gpu.py run those shapes through the wrappers.
"""

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _bounds as B  # noqa: E402
import _bounds_codec  # noqa: E402,F401

CASES = [c for c in B.CASES if c.build.__module__ == "_bounds_codec"]


@pytest.mark.parametrize("case", CASES, ids=[f"{c.entry[5:]}-{c.id}" for c in CASES])
def test_buffer_contract(dev, oracle, case):
    B.run_case(case, dev, oracle)

"""-m gpu: dqq_newton_active_f64's addressing past 2^32 bytes, in the manner of tests/test_gpu_jac_offsets.py with
tests/offset_cases.py's helpers: the team family with P past 2^32 bytes (N = 8), and DQQ_P_DIAG with every (B,N) buffer of the
call -- P, q, the bounds, v, x and mult -- past 2^32 bytes (N = 64; state, int32, is past 2^31 bytes).

Per row a base of nb problems (trip_cases.base_size: prime) is tiled on the device to B = ceil(2^29 / doubles per problem) +
2 nb + 1 problems: two whole replicas lie above the mark and the batch ends ragged.  ONE call, every output pre-filled with a
sentinel.  Then replica 0 is bit-equal to the host core, every problem b is bit-equal to problem b mod nb in every output, and
no sentinel is left in the last whole replica and the ragged tail.  An address that wraps reads another problem's data or leaves
an output above the mark unwritten.  A row skips only when the card has less free memory than it needs."""
import numpy as np
import pytest
import torch

import active_cases as C
import polish_cases as PC
import polish_reference as R
from offset_cases import M32, V32, batch, count_equal_bits, first_unequal_replica, per_problem
from trip_cases import base_size

pytestmark = pytest.mark.gpu
DENSE, DIAG = 1, 2
SENTINEL_BITS = 0x7FF8DEADBEEF0001        # a NaN no kernel produces
SENTINEL_INT = -7
MARGIN = 2 << 30
# (kind, N, layout, structure, mark)
ROWS = [("qcqp", 8, DENSE, "dense", M32), ("sbox", 64, DIAG, "diag", V32)]


@pytest.mark.parametrize("kind,N,layout,structure,mark", ROWS, ids=lambda v: str(v))
def test_addresses_past_the_mark(kind, N, layout, structure, mark):
    try:
        _run(kind, N, layout, structure, mark)
    except torch.cuda.OutOfMemoryError:
        raise
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("newton active offsets %s N=%d: %s" % (kind, N, e), returncode=3)


def _run(kind, N, layout, structure, mark):
    from diffqcqp_amd import _capi, build
    build.build()
    diag = layout == DIAG
    nb, B = base_size(N), batch(N, mark, layout)
    pp = per_problem(N, layout)
    ne = C.elements(kind, N)
    assert B * pp * 8 > 1 << 32 and B - -(-mark // pp) >= 2 * nb
    nex = len(PC.EXTRAS[kind])
    need = B * (8 * (pp + 2 * N + nex * ne + ne + 1) + 4 * (ne + 2) + 8) + MARGIN
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("needs %.2f GiB of device memory, %.2f GiB are free" % (need / 2 ** 30, free / 2 ** 30))
    P, q, ex, x = C.random_problem(kind, nb, N, structure)
    Pa = PC.compact(P) if diag else P
    ref = dict(zip(C.NAMES, C.host_active(kind, Pa, q, ex, x, diag=diag)))
    assert not ref["status"].any()
    cu = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()   # noqa: E731
    idx = torch.arange(B, device="cuda") % nb
    big = [cu(a).index_select(0, idx) for a in [Pa, q, *ex, x]]
    for t in big[:1] + ([] if not diag else big[1:]):      # what the row is about lies past 2^32 bytes
        assert t.numel() * 8 > 1 << 32
    f64 = lambda *s: torch.full(s, SENTINEL_BITS, dtype=torch.int64, device="cuda").view(torch.float64)   # noqa: E731
    i32 = lambda *s: torch.full(s, SENTINEL_INT, dtype=torch.int32, device="cuda")                         # noqa: E731
    out = {"state": i32(B, ne), "mult": f64(B, ne), "margin": f64(B), "where": i32(B), "status": i32(B)}
    assert not diag or (out["mult"].numel() * 8 > 1 << 32 and out["state"].numel() * 4 > 1 << 31)
    head = [R.KIND[kind]] + [t.data_ptr() for t in big[:2 + nex]] + [0] * (3 - nex) + [big[2 + nex].data_ptr()]
    rc = _capi.lib().dqq_newton_active_f64(*head, *[out[n].data_ptr() for n in C.NAMES], B, N, layout,
                                           torch.cuda.current_stream().cuda_stream)
    _capi.check(rc, "dqq_newton_active_f64")
    torch.cuda.synchronize()
    first = torch.arange(nb, device="cuda")
    for name, t in out.items():
        got = t[:nb].cpu().numpy()      # replica 0: the host core's bits
        assert got.dtype == ref[name].dtype and C.same_outputs([got], [ref[name]]) is None, name
        bad = first_unequal_replica(t, idx, first)      # every problem: the bits of its base problem
        assert bad is None, "%s of problem %d (base problem %d) differs from replica 0; %d problems differ" % (
            name, bad[0], bad[0] % nb, bad[1])
        left = count_equal_bits(t, B - B % nb - nb, SENTINEL_BITS if t.dtype == torch.float64 else SENTINEL_INT)
        assert left == 0, "%d entries of %s above problem %d were not written" % (left, name, B - B % nb - nb)
    print("%s N=%d layout %d: B %d, peak %.2f GiB" % (kind, N, layout, B, torch.cuda.max_memory_allocated() / 2 ** 30))
    del big, out, idx
    torch.cuda.empty_cache()

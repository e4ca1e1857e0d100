"""CPU checks of ops.newton_jacobian_jvp / ops.newton_jacobian_vjp (torch only, so CPU tensors do): the compact DQQ_P_DIAG form
against the same block-diagonal Jacobians written out as general ones, for every kind at N = 2 and 8 -- the QCQP at N = 2 with
Jq alone included, where the shapes cannot tell the two forms apart and `compact=True` has to say so."""
import pytest
import torch

KINDS = ("qp", "qcqp", "box", "sbox")
K, B = 3, 5


def _blocks(kind, N, g):
    """-> (compact (Jq, Ja, Jb), the same as general Jacobians), random block-diagonal."""
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    if kind != "qcqp":
        c = [r(B, N) for _ in range(1 if kind == "qp" else 3)]
        return tuple(c), tuple(torch.diag_embed(j) for j in c)
    cq, ca, cb = r(B, N, 2), r(B, N), r(B, N)
    fq = torch.block_diag(*[torch.zeros(2, 2)] * (N // 2)).to(torch.float64).repeat(B, 1, 1)
    fa, fb = torch.zeros(B, N, N // 2, dtype=torch.float64), torch.zeros(B, N, N // 2, dtype=torch.float64)
    for i in range(N):
        k = i // 2
        fq[:, i, 2 * k], fq[:, i, 2 * k + 1] = cq[:, i, 0], cq[:, i, 1]
        fa[:, i, k], fb[:, i, k] = ca[:, i], cb[:, i]
    return (cq, ca, cb), (fq, fa, fb)


@pytest.mark.parametrize("only_jq", [False, True])
@pytest.mark.parametrize("N", [2, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_compact_helpers_equal_the_general_ones(kind, N, only_jq):
    from diffqcqp_amd import ops
    g = torch.Generator().manual_seed(100 * N + KINDS.index(kind))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    c, f = _blocks(kind, N, g)
    if only_jq:
        c, f = (c[0],) + (None,) * (len(c) - 1), (f[0],) + (None,) * (len(f) - 1)
    ne = N // 2 if kind == "qcqp" else N
    x, gx = r(B, N, 1), r(K, B, N, 1)
    dPc, dq = r(K, B, N), r(K, B, N, 1)
    ext = (r(K, B, ne, 1), r(K, B, ne, 1)) if kind != "qp" and not only_jq else ()
    flag = True if (kind == "qcqp" and N == 2 and only_jq) else None      # the one case the shapes cannot tell
    dxc = ops.newton_jacobian_jvp(kind, c, x, (dPc, dq) + ext, compact=flag)
    dxf = ops.newton_jacobian_jvp(kind, f, x, (torch.diag_embed(dPc), dq) + ext)
    assert dxc.shape == (K, B, N, 1) and torch.allclose(dxc, dxf, rtol=0, atol=1e-13)
    vc = ops.newton_jacobian_vjp(kind, c, x, gx, compact=flag)
    vf = ops.newton_jacobian_vjp(kind, f, x, gx)
    assert vc[0].shape == (K, B, N) and vf[0].shape == (K, B, N, N)
    assert torch.allclose(vc[0], torch.diagonal(vf[0], dim1=2, dim2=3), rtol=0, atol=1e-13)
    for a, b in zip(vc[1:], vf[1:]):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape and torch.allclose(a, b, rtol=0, atol=1e-13)
    # the general form against plain index sums
    want = torch.einsum("bij,kbj->kbi", f[0], gx[:, :, :, 0].new_tensor(0) + (torch.diag_embed(dPc) @ x.unsqueeze(0))[..., 0] + dq[..., 0])
    if ext:
        want = want + torch.einsum("bij,kbj->kbi", f[1], ext[0][..., 0]) + torch.einsum("bij,kbj->kbi", f[2], ext[1][..., 0])
    assert torch.allclose(dxf[..., 0], want, rtol=0, atol=1e-13)
    assert torch.allclose(vf[1][..., 0], torch.einsum("bij,kbi->kbj", f[0], gx[..., 0]), rtol=0, atol=1e-13)

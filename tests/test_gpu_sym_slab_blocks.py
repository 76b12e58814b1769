"""k_sym_slab at every block count: the stacked group form (BIEM_SYM_UPDATE=left, BIEM_SYM_GROUP=stacked) at n_pad = 320 and 576 with
3 systems.  Every group with more than one panel launches the slab kernel with one, two and three blocks per system (panels b, c, d);
320 has one such group and a single panel behind it, 576 two and a single panel.  Factors and solutions agree with the two-pass form
(BIEM_SYM_GROUP=twopass) inside the bounds tests/test_gpu_sym_stacked_group.py applies to the same pair: 1e-12 of each system's
largest factor entry, 1e-12 relative on the solutions.  Generator and launcher are that module's.
"""
import pytest

import test_gpu_sym_stacked_group as G
from test_gpu_sym_stacked_group import lib, torch  # noqa: F401  (the module's fixture)

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("n_pad", [320, 576])
def test_slab_blocks_against_two_pass(lib, monkeypatch, n_pad):  # noqa: F811
    l, L = lib
    nb, nrhs, seed = 3, 2, 7300 + n_pad
    upper = ~G._lower_tiles(n_pad)
    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    U, X = {}, {}
    for group in G.GROUP_FORMS:
        A, info = G._factor_solve(l, L, monkeypatch, group, n_pad, nb, nrhs, seed)
        assert (info == 0).all(), (group, info.tolist())
        U[group], X[group] = A[:, :, :n_pad].clone(), A[:, :, n_pad:n_pad + nrhs].clone()
    du = torch.where(upper, (U["stacked"] - U["twopass"]).abs(), zero).amax(dim=(1, 2)) / torch.where(upper, U["twopass"].abs(), zero).amax(dim=(1, 2))
    dx = (X["stacked"] - X["twopass"]).abs().amax(dim=(1, 2)) / X["twopass"].abs().amax(dim=(1, 2))
    print(f"n_pad {n_pad}: factors {du.max().item():.3e}, solutions {dx.max().item():.3e}")
    assert (du < 1e-12).all(), du.tolist()
    assert (dx < 1e-12).all(), dx.tolist()
    assert not torch.equal(U["stacked"], U["twopass"])          # different arithmetic: the switch is seen to switch

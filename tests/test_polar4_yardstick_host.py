"""tests/polar4_yardstick.py against what pins it (no GPU).

1. Its polar triple integrals (float64, 3 n_end + 3 nodes) against the 40-digit values of tests/golden/polar4_integrals.npz on every
   stored triple: bba at n_end 15, 18, 22, 24, caa at 13, 14 (either side of the general fill's pair-table switch) and 26, 27 (the first
   order whose top block holds non-vanishing integrals below 1e-13, and the next).  The largest difference is the accuracy float64
   reaches; it is printed, and bounded by POLAR_FP64_ACCURACY, from which tests/test_polar4_terms_host.py takes its tolerance.
2. Its assembled coefficients against `chain_yardstick.gaunt(4, 6)` (bba) and `O._theta_c(6)` (caa), both pinned by the reference goldens.
"""
import os

import numpy as np
import pytest

from oracle import biem_oracle as O

import chain_yardstick as CY
import polar4_yardstick as PY

FIXTURE = np.load(os.path.join(os.path.dirname(__file__), "golden", "polar4_integrals.npz"))
CASES = [("bba", 15), ("bba", 18), ("bba", 22), ("bba", 24), ("caa", 13), ("caa", 14), ("caa", 26), ("caa", 27)]
# The accuracy of the float64 integrals, as measured by test 1: 2.9e-14 at bba n_end 24 (on an integral of modulus 1.4; 1.6e-14 at 22,
# 1.3e-14 at 18, 8.4e-15 at 15) and 7e-15 .. 9e-15 for caa; BASELINE.md holds the figures.  The size is what the arithmetic predicts: a
# node value comes from a three-term recurrence of up to 2 n_end steps and each integral sums 3 n_end + 3 products of three such
# values with sum |w a b c| of order one - some tens of 2.2e-16 times the order.
POLAR_FP64_ACCURACY = 3e-14


def fixture_case(tree, n_end):
    key = f"{tree}_{n_end}_"
    return FIXTURE[key + "lab"].astype(np.int64), FIXTURE[key + "val"], FIXTURE[key + "zero"], FIXTURE[key + "pairs"].astype(np.int64)


def twin_values(tree, n_end, lab):
    y = (PY.Bba if tree == "bba" else PY.Caa)(n_end)
    out = np.zeros(len(lab))
    for i, r in enumerate(lab.tolist()):
        if tree == "bba":
            out[i] = y.polar(*r[:4])[r[4], r[5]]
        else:
            q3, v = y.polar(*r[:6], r[7], r[8])
            out[i] = v[(r[6] - r[7] - r[8]) // 2]
    return out


def test_fixture_holds_every_case():
    assert sorted({k.rsplit("_", 1)[0] for k in FIXTURE.files}) == sorted(f"{t}_{n}" for t, n in CASES)


@pytest.mark.parametrize("tree,n_end", CASES)
def test_twin_equals_the_40_digit_integrals(tree, n_end):
    lab, val, zero, pairs = fixture_case(tree, n_end)
    assert len(lab) == len(val) == len(zero) > 1000 and len(pairs) >= 30
    assert (val[zero] == 0).all() and (np.abs(val[~zero]) >= 1e-30).all()
    got = twin_values(tree, n_end, lab)
    err = np.abs(got - val)
    live = np.abs(val[~zero])
    print(f"{tree} n_end {n_end}: {len(lab)} integrals, {int((~zero).sum())} do not vanish (smallest {live.min():.3e}, {int((live < 1e-12).sum())} "
          f"below 1e-12); max |twin - fixture| {err[~zero].max():.2e} on those, {err[zero].max():.2e} on the vanishing ones")
    assert err.max() <= POLAR_FP64_ACCURACY, (tree, n_end, lab[err.argmax()], err.max())


def test_bba_coefficients_equal_the_chain_yardstick_at_n_end_6():
    y, g = PY.Bba(6), CY.gaunt(4, 6)
    assert y.idx == g.idx and y.idx2 == g.idx2
    worst = 0.0
    for hp in range(0, y.H, 2):
        for h in range(y.H):
            c1, g1 = g.all_labels(hp, h)
            want = np.zeros(y.H2)
            want[c1] = np.real(1j ** ((g.idx[h][0] + g.deg2[c1] - g.idx[hp][0]) % 4)) * g1
            worst = max(worst, np.abs(PY.coefficients(y, hp, h) - want).max())
    print(f"bba n_end 6: max |twin - chain yardstick| over {y.H * ((y.H + 1) // 2)} entries, every label: {worst:.2e}")
    assert worst <= 1e-13


def test_caa_coefficients_equal_theta_c_at_n_end_6():
    y, I3 = PY.Caa(6), O._theta_c(6)
    worst = 0.0
    for hp, (qp, m1p, m2p) in enumerate(y.idx):
        for h, (q, m1, m2) in enumerate(y.idx):
            coef = PY.coefficients(y, hp, h)
            want = np.zeros(y.H2)
            mu1, mu2 = m1p - m1, m2p - m2
            for q3 in range(abs(q - qp), q + qp + 1, 2):
                if q3 >= abs(mu1) + abs(mu2):
                    want[y.pos2[(q3, mu1, mu2)]] = np.real(1j ** ((q + q3 - qp) % 4)) * I3.get(qp, abs(m1p), abs(m2p), q, abs(m1), abs(m2), q3, abs(mu1), abs(mu2)) / (2 * np.pi)
            worst = max(worst, np.abs(coef - want).max())
    print(f"caa n_end 6: max |twin - theta_c / 2 pi| over {y.H ** 2} entries, every label: {worst:.2e}")
    assert worst <= 1e-13

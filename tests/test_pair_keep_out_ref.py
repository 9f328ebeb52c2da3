"""The yardstick of the vehicle-pair separation rows (tests/pair_keep_out_ref.py) held to itself, without a device: its two-sided
block against its own forward differences, the symmetry of the rows under a swap of the two vehicles, and the conditions the GPU
tests of tests/test_gpu_pair_keep_out.py rely on (negative rows, searches that split, generic rows of the provider inputs).
The regions go through the Python layer's own check (optimization._separation_region_table), as they do on their way to the
device.  DESIGN.md 4.27."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_keep_out_ref as ref  # noqa: E402

ALL_REGIONS = [(dim, name) for dim in (2, 3) for name, _ in ref.REGIONS[dim]]


def _table(dim, name):
    """the region's H as BezOptimization hands it to the device"""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    H = dict(ref.REGIONS[dim])[name]()
    T = opt._separation_region_table((H[:, :dim], H[:, dim]), dim)
    assert np.array_equal(T, H)
    return T


@pytest.mark.parametrize("dim,name", ALL_REGIONS)
def test_block_against_forward_differences(dim, name):
    """h = 1e-6, eps_rel = 1e-12, acceptance 1e-4, on BOTH vehicles' control points: the first vehicle's block is
    the block of D, the second's its negation.  Generic rows of the first two batch rows at degrees 3 and 5, both metrics."""
    H = _table(dim, name)
    for metric in ref.METRICS:
        reg = ref.Region(H, metric)
        worst, compared = 0.0, 0
        for deg in (3, 5):
            Y = ref.batch(deg, dim, ref.seed_of(deg, dim))
            for b in range(2):
                V = ref.vehicles(Y[b], ref.N_VEH)
                for i, j in zip(*ref.pairs(ref.N_VEH)):
                    if not reg.generic(ref.relative(V[i], V[j])):
                        continue
                    bi, bj, _ = ref.two_sided_block(V[i], V[j], reg)
                    fi, fj = ref.forward_difference(V[i], V[j], reg)
                    assert np.array_equal(bj, -bi)
                    gap = max(float(np.abs(bi - fi).max()), float(np.abs(bj - fj).max()))
                    worst, compared = max(worst, gap), compared + 1
                    assert gap <= 1e-4, (name, metric, deg, b, int(i), int(j), gap)
        print("%s, %s: largest |block - forward difference| %.3e over %d generic rows, both sides" % (name, metric, worst, compared))
        assert compared >= 6


@pytest.mark.parametrize("dim,name", ALL_REGIONS)
def test_swap_symmetry(dim, name):
    """R = -R: swapping the two vehicles leaves the row unchanged (every face has its mirror image, so the coefficients of -D are
    those of D with the faces renamed).  The triangle and the tetrahedron: some row changes."""
    H = _table(dim, name)
    deg = 5
    Y = ref.batch(deg, dim, ref.seed_of(deg, dim))
    for metric in ref.METRICS:
        reg = ref.Region(H, metric)
        changed = 0
        for b in range(ref.B_ROWS):
            V = ref.vehicles(Y[b], ref.N_VEH)
            for i, j in zip(*ref.pairs(ref.N_VEH)):
                a, c = reg.search(ref.relative(V[i], V[j]))["val"], reg.search(ref.relative(V[j], V[i]))["val"]
                if name in ref.SYMMETRIC:
                    assert abs(a - c) <= 1e-12 * max(1.0, abs(a)), (name, metric, b, int(i), int(j), a, c)
                else:
                    changed += abs(a - c) > 1e-6
        if name not in ref.SYMMETRIC:
            print("%s, %s: %d of %d rows change when the two vehicles are swapped" % (name, metric, changed, ref.B_ROWS * 6))
            assert changed > 0


@pytest.mark.parametrize("dim", (2, 3))
def test_batches_hold_what_the_gpu_tests_need(dim):
    """Per metric, region and degree: no search runs out of budget, at least one row is negative, one positive, and one search
    splits (nodes > 1) -- what test_gpu_pair_keep_out.py's identity test asks of its batches."""
    for name, _ in ref.REGIONS[dim]:
        H = _table(dim, name)
        for metric in ref.METRICS:
            reg = ref.Region(H, metric)
            for deg in ref.DEGREES:
                Y = ref.batch(deg, dim, ref.seed_of(deg, dim))
                rs = [r for b in range(ref.B_ROWS) for r in ref.rows(Y[b], ref.N_VEH, reg)]
                assert len(rs) == 30 and all(r["ok"] for r in rs)
                neg, pos, split = (sum(r["val"] < 0 for r in rs), sum(r["val"] > 0 for r in rs), sum(r["nodes"] > 1 for r in rs))
                print("%s, %s, degree %d: %d negative, %d positive, %d searches split" % (name, metric, deg, neg, pos, split))
                assert neg >= 1 and pos >= 1 and split >= 1


@pytest.mark.parametrize("name", sorted(ref.PROBLEMS))
def test_genericity_counts(name):
    """The provider inputs of the GPU tests: how many rows the yardstick calls generic (one minimum, not within 1e-3 of a second,
    |val| >= 1e-3), under both metrics -- at least half, so that the envelope-against-fd comparison there covers at least half."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    for metric in ref.METRICS:
        bo, x = ref.provider_input(name, separationRegionMetric=metric)
        Nv, dim = bo.model['numVeh'], bo.model['dim']
        reg = ref.Region(opt._separation_region_table(bo.separationRegion, dim), metric)
        rs = ref.rows(bo.reshapeVector(x), Nv, reg)
        gen = [reg.generic(r["D"]) for r in rs]
        print("%s, %s: rows %s, generic %d of %d" % (name, metric, [round(r["val"], 4) for r in rs], sum(gen), len(gen)))
        assert len(rs) == Nv * (Nv - 1) // 2 and 2 * sum(gen) >= len(gen)

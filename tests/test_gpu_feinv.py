"""GPU: the safegcd inverse (csrc/feinv.hpp) as the device compiler builds it.  Piecewise: divsteps30, divsteps30_var, update_de, update_fg,
normalize and the two conversions by a kernel (pk_probe_inv30_device, one lane per record) on the records of tests/feinv_refs.py -- the
matrices with |u| + |v| = 2^30, d and e at both ends of (-2p, p), md at both ends of its range, whole batches of zeros, swaps at the
first and last steps -- device == definition, host == definition, device == host, each stated on its own so that a failure names the
side.  Whole: ops 21-23 on operands whose walks leave the middle of the road, in two lane orders (sorted by batches taken; and with the
lanes that leave fe_inverse_plain_var's loop first next to the ones that leave it last, in every wavefront), and the witness kernel's own
instantiation (OP_INVERSE) on the same lanes.  tests/test_feinv_host.py is the CPU half and holds the operand sets to what they must reach."""
import numpy as np
import pytest

import feinv_refs as fr

pytestmark = pytest.mark.gpu

P = fr.P


def part_host_and_device(ctx, part, rin):
    from provekit_amd._lib import lib
    from tools.pk_probes import lib as probes

    rin = np.ascontiguousarray(rin, dtype=np.int32)
    n = rin.shape[0]
    host = np.full_like(rin, -1)
    assert lib.pk_selftest_inv30(part, rin.ctypes.data, host.ctypes.data, n) == 0
    d_in, d_out = ctx.upload(rin), ctx.alloc(rin.nbytes)
    ctx._check(probes.pk_probe_inv30_device(ctx.handle, part, d_in.ptr, d_out.ptr, n))
    return host, ctx.download(d_out, rin.shape, np.int32)


def arith_host_and_device(ctx, op, xs):
    from provekit_amd._lib import lib
    from tools.pk_probes import lib as probes

    a = fr.to_limbs(xs)
    n = a.shape[0]
    host = np.empty_like(a)
    assert lib.pk_selftest_arith(op, a.ctypes.data, a.ctypes.data, host.ctypes.data, n) == 0
    da, do = ctx.upload(a), ctx.alloc_fe(n)
    ctx._check(probes.pk_probe_arith_device(ctx.handle, op, da.ptr, da.ptr, do.ptr, n))
    return fr.from_limbs(host), fr.from_limbs(ctx.download_fe(do, n))


def wrong(got, want, xs):
    return [(i, hex(x), hex(g), hex(w)) for i, (x, g, w) in enumerate(zip(xs, got, want)) if g != w][:4]


@pytest.mark.parametrize("part", sorted(fr.PARTS))
def test_every_part_device_host_and_definition_agree(ctx, part):
    rin, want = fr.records(part)
    host, dev = part_host_and_device(ctx, part, rin)
    name = fr.PARTS[part]
    assert fr.differing(dev, want, rin) == [], f"{name}: the device build differs from the definition"
    assert fr.differing(host, want, rin) == [], f"{name}: the host build differs from the definition"
    assert np.array_equal(dev, host)
    if part in (2, 3, 4):  # limbs 0..7 of every result are canonical
        low = np.delete(dev[:, :18], [8, 17], axis=1)
        assert low.min() >= 0 and low.max() < fr.B30


def test_a_refused_part_launches_nothing(ctx):
    from tools.pk_probes import lib as probes

    rin = fr.records(0)[0][:64]
    d_in, d_out = ctx.upload(rin), ctx.alloc(rin.nbytes)
    for part in (-1, 7):
        assert probes.pk_probe_inv30_device(ctx.handle, part, d_in.ptr, d_out.ptr, 64) != 0


@pytest.mark.parametrize("order", ["sorted", "interleaved"])
@pytest.mark.parametrize("op", [21, 22, 23])
def test_the_whole_inverse_in_both_lane_orders(ctx, op, order):
    """sorted: the lanes of a wavefront leave the variable-time loop together; interleaved: a lane that takes no batch and lanes that take
    the fewest sit next to lanes that take the most, in every wavefront.  op 21 is fed the values themselves (as Montgomery images), so
    that the walk inside is the listed one: x^-1 R^2."""
    xs = fr.sorted_order() if order == "sorted" else fr.interleaved_order()
    assert len(xs) > 1000
    want = [fr.inverse(x) * (fr.R * fr.R if op == 21 else 1) % P for x in xs]
    host, dev = arith_host_and_device(ctx, op, xs)
    assert wrong(dev, want, xs) == [], "the device build differs from pow(x, -1, p)"
    assert wrong(host, want, xs) == [], "the host build differs from pow(x, -1, p)"
    assert dev == host


def test_the_witness_kernels_inverse_on_the_interleaved_lanes(ctx, oracle):
    """csrc/witness.hip's own instantiation (OP_INVERSE -> fe_inverse_mont): one Acir input and one Inverse per non-zero value of the list,
    in the interleaved order (18 wavefronts of one level), against the sequential solver.  The ACIR value is x R^-1, so that its
    Montgomery image -- what fe_inverse_plain_var walks -- is the listed x."""
    from test_gpu_witness import _check

    from provekit_amd.witness import WitnessBuilder as WB

    xs = [x for x in fr.interleaved_order() if x]
    n = len(xs)
    assert n > 1000
    rinv = pow(fr.R, -1, P)
    acir = [x * rinv % P for x in xs]
    builders = [WB.Acir(i, i) for i in range(n)] + [WB.Inverse(n + i, i) for i in range(n)]
    want = _check(ctx, oracle, builders, acir, [], 2 * n)
    assert want[n:] == [fr.inverse(a) for a in acir]

"""GPU: the field's carry chains as the device compiler builds them, on the operands of tests/fe_carry_cases.py (carries riding
through all-ones words, borrows riding through equal words, sums, differences and products landing on and next to the modulus):
device bits == host bits == Python ints, every comparison stated on its own so that a failure names the side that is wrong.
tests/test_fe_carry_host.py is the CPU half."""
import numpy as np
import pytest

import fe_carry_cases as fc

pytestmark = pytest.mark.gpu

P = fc.P


def host_and_device(ctx, op, xs, ys):
    from provekit_amd._lib import lib
    from tools.pk_probes import lib as probes

    a, b = fc.to_limbs(xs), fc.to_limbs(ys)
    n = a.shape[0]
    host = np.empty_like(a)
    assert lib.pk_selftest_arith(op, a.ctypes.data, b.ctypes.data, host.ctypes.data, n) == 0
    da, db, do = ctx.upload(a), ctx.upload(b), ctx.alloc_fe(n)
    ctx._check(probes.pk_probe_arith_device(ctx.handle, op, da.ptr, db.ptr, do.ptr, n))
    return fc.from_limbs(host), fc.from_limbs(ctx.download_fe(do, n))


def wrong(got, want, xs, ys):
    return [(hex(x), hex(y), hex(g), hex(w)) for x, y, g, w in zip(xs, ys, got, want) if g != w][:4]


@pytest.mark.parametrize("op", sorted(fc.NEW_OPS))
def test_chain_op_device_host_and_ints_agree(ctx, op):
    xs, ys, want = fc.new_op_cases(op)
    host, dev = host_and_device(ctx, op, xs, ys)
    name = fc.NEW_OPS[op][0]
    assert wrong(dev, want, xs, ys) == [], f"{name}: the device build differs from the definition"
    assert wrong(host, want, xs, ys) == [], f"{name}: the host build differs from the definition"
    assert dev == host


@pytest.mark.parametrize("name", ["add", "sub", "mul"])
def test_elementwise_kernels_on_the_carry_pairs(ctx, name):
    """pk_fe_add / pk_fe_sub / pk_fe_mul through the C ABI: the elementwise kernel's own instantiation of the chains"""
    from provekit_amd._lib import lib

    pairs = {"add": fc.add_pairs() + fc.sub_pairs(), "sub": fc.sub_pairs() + fc.add_pairs(),
             "mul": tuple((x, y) for x, y, _ in fc.mont_products()) + fc.limb_add_pairs()}[name]
    define = {"add": lambda x, y: (x + y) % P, "sub": lambda x, y: (x - y) % P, "mul": lambda x, y: x * y * fc.RINV % P}[name]
    xs, ys = [x for x, _ in pairs], [y for _, y in pairs]
    n = len(xs)
    da, db, do = ctx.upload(fc.to_limbs(xs)), ctx.upload(fc.to_limbs(ys)), ctx.alloc_fe(n)
    ctx._check(getattr(lib, f"pk_fe_{name}")(ctx.handle, da.ptr, db.ptr, do.ptr, n))
    assert wrong(fc.from_limbs(ctx.download_fe(do, n)), [define(x, y) for x, y in pairs], xs, ys) == []


def test_wide_reduce_device_equals_host_on_every_multiple_of_p(ctx):
    cases = fc.wide_pairs()
    xs, ys = [c[0] for c in cases], [c[1] for c in cases]
    want = [d % P for _, _, _, d in cases]
    host, dev = host_and_device(ctx, 14, xs, ys)
    assert wrong(dev, want, xs, ys) == [], "wide_reduce: the device build differs from the definition"
    assert wrong(host, want, xs, ys) == [], "wide_reduce: the host build differs from the definition"
    assert dev == host


@pytest.mark.parametrize("op", [0, 24])
def test_targeted_products_device_equals_host(ctx, op):
    cases = fc.mont_products() if op == 0 else fc.shoup_products()
    xs, ys, ts = ([c[i] for c in cases] for i in range(3))
    host, dev = host_and_device(ctx, op, xs, ys)
    assert wrong(dev, ts, xs, ys) == [], "the device build differs from the definition"
    assert wrong(host, ts, xs, ys) == [], "the host build differs from the definition"
    assert dev == host


@pytest.mark.parametrize("op", sorted(fc.OLD_UNARY))
def test_single_operand_ops_device_equals_host_on_the_structured_values(ctx, op):
    _, define = fc.OLD_UNARY[op]
    xs = fc.old_unary_cases(op)
    host, dev = host_and_device(ctx, op, xs, xs)
    if define is None:  # op 9: almost reduced; the bits are still the host's
        assert all(r % P == x % P and r < P + (P >> 10) for x, r in zip(xs, dev))
    else:
        want = [define(x) for x in xs]
        assert wrong(dev, want, xs, xs) == [], "the device build differs from the definition"
        assert wrong(host, want, xs, xs) == [], "the host build differs from the definition"
    assert dev == host

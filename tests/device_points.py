"""Uniformly random points for the GPU suites: [k_i]G of device-resident scalars
k_i.  BN254 and BLS12-377 take the device's own fixed-base multiplication;
gm_batch_mul_base refuses BLS12-381 (a deferred entry), so that curve's points
come from the C++ oracle's table on the host and are copied in.  The curve is
the only thing the branch looks at."""
import gnark_mi355x as gm
import oracle_lib


def batch_mul_generator(ctx, cname, g2, K, n):
    """Device buffer of the n points [K_i]G (gnark layout), G the group's generator."""
    if cname == "bls12381":
        host = oracle_lib.batch_mul_base(cname, g2, oracle_lib.generator(cname, g2), K.to_host(32 * n))
        return ctx.copy_to_device(host)
    return ctx.batch_mul_base(cname, g2, gm.generator(cname, g2), K, n)


def random_points_host(ctx, cname, g2, n, seed):
    """Host bytes of n random points: [k_i]G for random_scalars(seed)."""
    K = ctx.random_scalars(cname, n, seed)
    P = batch_mul_generator(ctx, cname, g2, K, n)
    out = P.to_host()
    K.free()
    P.free()
    return out

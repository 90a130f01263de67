"""Search the adversarial steering fixture tests/golden/phase_boundary.npz (run once, takes minutes; not a test).

    python tests/golden/make_phase_fixture.py [chunks]

Our own search over oracle/ (no reference code runs): the definitions are tests/phase_cases.py's.

1. Draw (tau, phi) as float32, |tau| <= 5.5e4 samples of either sign and phi in +-pi (the array_low / array_top
   model), zero rates, t0 = 0, and evaluate every draw at the 8 channels at the top of a 4096-channel L-band.
2. v = cos and v = sin of oracle.coeff_rotation in float64.
3. Keep (tau, phi, channel) when mag < 2e5 and the contract's word changes within the band,
   Qc(v - 2e-10) != Qc(v + 2e-10), Qc(v) = rint(2^14 float32(v)): a float32 rounding midpoint next to a Q14 boundary.
4. Mark the teeth: entries whose word differs when the rotation is formed the fast way, (tau chc) K + phi.
A second set does the same with a weight g of phase_cases.FIX_GAINS (draw i takes weight i mod 4) on
rint(RN32(RN32(v) g) 2^14).

The search evaluates cos / sin with NumPy; every candidate is then re-examined with libm (math.cos / math.sin, the
contract's evaluator, as tests/test_phase_cases_host.py does) and only entries that meet the definition there are
stored.  Stored: every tooth, then entries in search order up to 2048; 512 weighted ones.  Data only:
tau, phi (float32), channel (int16), is_tooth (bool); w_tau, w_phi, w_channel, w_gain, w_is_tooth.
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import oracle as O  # noqa: E402
import phase_cases as PC  # noqa: E402

DRAWS = 400_000  # per chunk, each at 8 channels
WEIGHTED_CHUNKS = 24
KEEP, KEEP_WEIGHTED = 2048, 512


def candidates(seed_and_index):
    seed, index = seed_and_index
    rng = np.random.default_rng(seed)
    reg = PC.FIX
    d = np.zeros((1, 1, DRAWS, 4), np.float32)
    d[0, 0, :, 0] = rng.uniform(-reg.tau_hi, reg.tau_hi, DRAWS) * reg.Ts
    d[0, 0, :, 2] = rng.uniform(-np.pi, np.pi, DRAWS)
    rot = O.coeff_rotation(np.broadcast_to(d, (PC.FIX_C, 1, DRAWS, 4)), PC.FIX_C, reg.Ctot, PC.FIX_XENG, reg.Ts)[:, 0]
    c, s = np.cos(rot), np.sin(rot)
    out = []
    gains = PC.FIX_GAINS[np.arange(DRAWS) % len(PC.FIX_GAINS)]
    for g in ([None, gains] if index < WEIGHTED_CHUNKS else [None]):
        near = PC.decision_within_band(c, g) | PC.decision_within_band(s, g)
        ci, di = np.nonzero(near)
        out.append((d[0, 0, di, 0], d[0, 0, di, 2], (PC.FIX_CH0 + ci).astype(np.int16),
                    None if g is None else g[di]))
    return out


def main():
    chunks = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    seeds = np.random.SeedSequence(20261021).spawn(chunks)
    sets = ([], [])
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for n, found in enumerate(pool.imap(candidates, zip(seeds, range(chunks)))):
            for k, f in enumerate(found):
                sets[k].append(f)
            if n % 20 == 19:
                print(f"{n + 1} chunks: {sum(len(f[0]) for f in sets[0])} candidates", flush=True)
    z = {}
    for k, (prefix, keep) in enumerate((("", KEEP), ("w_", KEEP_WEIGHTED))):
        tau, phi, ch = (np.concatenate([f[j] for f in sets[k]]) for j in range(3))
        g = np.concatenate([f[3] for f in sets[k]]) if k else None
        kept, tooth, diff = PC.fixture_flags(tau, phi, ch, g)  # by libm: the definition
        print(f"{prefix or 'unit'}: {len(tau)} candidates, {int(kept.sum())} meet the definition by libm, "
              f"{int((kept & tooth).sum())} teeth, max |fast - ref| {diff[kept].max():.3g} rad "
              f"(teeth {diff[kept & tooth].max() if (kept & tooth).any() else 0:.3g})")
        order = np.concatenate([np.flatnonzero(kept & tooth), np.flatnonzero(kept & ~tooth)])[:keep]
        order.sort()
        z[prefix + "tau"], z[prefix + "phi"], z[prefix + "channel"] = tau[order], phi[order], ch[order]
        z[prefix + "is_tooth"] = tooth[order]
        if k:
            z["w_gain"] = g[order].astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "phase_boundary.npz"), **z)
    print({k: (v.shape, str(v.dtype)) for k, v in z.items()}, "draws x channels:", chunks * DRAWS * PC.FIX_C)


if __name__ == "__main__":
    main()

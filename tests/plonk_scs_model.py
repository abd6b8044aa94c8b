"""The model the gm_plonk_scs_* tests compare against, written from gnark's
definitions and never calling the library under test:

  * tables(): evaluateLROSmallDomain's row convention (constraint/bls12-377/
    system.go): rows (i, 0, 0) for the public inputs, the constraints from row
    nb_public on, (0, 0, 0) padding;
  * selectors(): NewTrace's loop (backend/plonk/bls12-377/setup.go:153-213) in
    Python integers, and selector_bytes(): the same columns as the bytes the
    device must write, by a numpy gather of the encoded CoeffTable;
  * unsatisfied(): the gate equation ql l + qr r + qm l r + qo o + qk in Python
    integers on the records gnark's solver checks (Commitment == NOT);
  * two generators: random circuits, and a satisfiable chain with its witness.

A record is gnark's constraint.SparseR1C as it lies in memory: nine u32,
XA XB XC QL QR QO QM QC Commitment."""
import random
import types

import numpy as np

XA, XB, XC, QL, QR, QO, QM, QC, COMMITMENT = range(9)
NOT, COMMITTED, COMMITMENT_ROW = 0, 1, 2  # constraint.CommitmentConstraint
# the order of gm_plonk_scs_selector's columns, as record fields
SELECTOR_FIELDS = (QL, QR, QM, QO, QC)
SELECTOR_NAMES = ("ql", "qr", "qm", "qo", "qk")


def enc(c, vals):
    """gnark's Montgomery words of integers mod r."""
    r, R = c.r, 1 << 256
    return b"".join([(v % r * R % r).to_bytes(32, "little") for v in vals])


def tables(records, n, nb_public):
    """The three wire-id columns, n rows each."""
    rec = np.asarray(records, np.uint32).reshape(-1, 9)
    t = np.zeros((3, n), np.uint32)
    t[0, :nb_public] = np.arange(nb_public)
    t[:, nb_public:nb_public + len(rec)] = rec[:, :3].T
    return t


def selectors(c, records, coeffs, n, nb_public, committed=()):
    """NewTrace: {"ql": [...], ..., "qk": [...]} and the list of qcp columns, as
    integers mod r, Lagrange regular (qk incomplete)."""
    r = c.r
    cols = {k: [0] * n for k in SELECTOR_NAMES}
    for i in range(nb_public):
        cols["ql"][i] = r - 1
    for i, rec in enumerate(np.asarray(records, np.uint32).reshape(-1, 9).tolist()):
        for name, field in zip(SELECTOR_NAMES, SELECTOR_FIELDS):
            cols[name][nb_public + i] = coeffs[rec[field]] % r
    qcp = []
    for rows in committed:
        q = [0] * n
        for i in rows:
            q[nb_public + int(i)] = 1
        qcp.append(q)
    return cols, qcp


def selector_bytes(c, records, coeffs, n, nb_public, committed=()):
    """The 5 + nb_bsb columns as (n, 32) uint8 arrays, in gm_plonk_scs_selector's order."""
    rec = np.asarray(records, np.uint32).reshape(-1, 9)
    table = np.frombuffer(enc(c, coeffs), np.uint8).reshape(len(coeffs), 32)
    one = np.frombuffer(enc(c, [1]), np.uint8)
    out = []
    for field in SELECTOR_FIELDS:
        col = np.zeros((n, 32), np.uint8)
        if field == QL:
            col[:nb_public] = np.frombuffer(enc(c, [c.r - 1]), np.uint8)
        col[nb_public:nb_public + len(rec)] = table[rec[:, field]]
        out.append(col)
    for rows in committed:
        col = np.zeros((n, 32), np.uint8)
        col[nb_public + np.asarray(rows, np.int64)] = one
        out.append(col)
    return out


def unsatisfied(c, records, coeffs, witness):
    """Indices of the constraints gnark's solver would reject."""
    r = c.r
    bad = []
    for i, rec in enumerate(np.asarray(records, np.uint32).reshape(-1, 9).tolist()):
        if rec[COMMITMENT] != NOT:
            continue
        l, rr, o = witness[rec[XA]], witness[rec[XB]], witness[rec[XC]]
        q = [coeffs[rec[k]] for k in (QL, QR, QM, QO, QC)]
        if (q[0] * l + q[1] * rr + q[2] * l * rr + q[3] * o + q[4]) % r:
            bad.append(i)
    return bad


def coeff_table(c, ncoeffs, rng):
    """gnark's CoeffTable: 0, 1, 2, -1, -2, then the circuit's own."""
    r = c.r
    head = [0, 1, 2, r - 1, r - 2]
    return (head + [rng.randrange(r) for _ in range(max(ncoeffs - 5, 0))])[:ncoeffs]


def random_circuit(c, n, nb_public, nb_constraints, nb_wires, ncoeffs, seed, nb_bsb=0):
    """Random records; coefficient ids 0 and ncoeffs - 1 and wires 0 and nb_wires - 1
    all occur (when there is a constraint to hold them).  With nb_bsb gates: a few
    COMMITTED rows per gate (one index twice) and one COMMITMENT row each."""
    rng = np.random.default_rng(seed)
    nc = nb_constraints
    rec = np.zeros((nc, 9), np.uint32)
    rec[:, :3] = rng.integers(0, nb_wires, size=(nc, 3))
    rec[:, 3:8] = rng.integers(0, ncoeffs, size=(nc, 5))
    if nc:
        rec[0, XA], rec[nc - 1, XC] = nb_wires - 1, 0
        rec[0, QL], rec[nc - 1, QC] = ncoeffs - 1, 0
        rec[nc // 2, XB], rec[nc // 2, QM] = 0, ncoeffs - 1
    committed, index = [], []
    for j in range(nb_bsb):
        index.append(1 + 2 * j)  # rows nb_public + 1, nb_public + 3
        rows = rng.choice(nc, size=min(4, nc), replace=False).astype(np.uint32)
        rows = np.r_[rows, rows[:1]]  # a duplicate: written twice
        committed.append(rows)
        rec[rows, COMMITMENT] = COMMITTED
    for i in index:
        rec[i, COMMITMENT] = COMMITMENT_ROW
    coeffs = coeff_table(c, ncoeffs, random.Random(seed))
    return types.SimpleNamespace(c=c, n=n, nb_public=nb_public, nb_constraints=nc, nb_wires=nb_wires,
                                 records=rec, coeffs=coeffs, committed=committed, commitment_index=index)


def chain_circuit(c, n, nb_public, nb_constraints, seed, ncoeffs=12, commitments=False):
    """A satisfiable circuit: x_(k+1) = a x_k x_(k-1) + b x_k + c, one constraint per
    step with l = x_k, r = x_(k-1), o = x_(k+1), qm = a, ql = b, qo = -1, qk = c
    and a, b, c drawn from the CoeffTable per row.  Wires 0 and 1 are x_0 and x_1
    (public inputs when nb_public >= 2).  commitments: constraint 1 becomes a
    COMMITMENT row and constraints 2, 5 COMMITTED rows whose equations do not hold
    (the solver does not look at them); their outputs are free wires, so the
    chain goes on.  Returns the circuit with .witness (integers)."""
    r = c.r
    rng = random.Random(seed)
    coeffs = coeff_table(c, ncoeffs, rng)
    nc = nb_constraints
    first = max(nb_public, 2)
    nb_wires = first + nc
    wit = [rng.randrange(r) for _ in range(first)] + [0] * nc
    rec = np.zeros((nc, 9), np.uint32)
    special = {1: COMMITMENT_ROW, 2: COMMITTED, 5: COMMITTED} if commitments else {}
    wire = lambda k: k if k < 2 else first + k - 2  # x_k
    for k in range(nc):
        a, b, cc = (rng.randrange(4, ncoeffs) for _ in range(3))
        xl, xr, xo = wire(k + 1), wire(k), wire(k + 2)
        rec[k] = (xl, xr, xo, b, 0, 3, a, cc, special.get(k, NOT))
        wit[xo] = (coeffs[a] * wit[xl] * wit[xr] + coeffs[b] * wit[xl] + coeffs[cc]) % r
        if k in special:
            wit[xo] = (wit[xo] + 1 + k) % r  # the equation fails here, and nobody minds
    committed = [np.array([2, 5], np.uint32)] if commitments else []
    index = [1] if commitments else []
    out = types.SimpleNamespace(c=c, n=n, nb_public=nb_public, nb_constraints=nc, nb_wires=nb_wires, records=rec,
                                coeffs=coeffs, committed=committed, commitment_index=index, witness=wit)
    assert unsatisfied(c, rec, coeffs, wit) == []
    return out

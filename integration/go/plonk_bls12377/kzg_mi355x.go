//go:build icicle

// GPU hooks for the BLS12-377 PLONK prover (BASELINE configs[4] "PLONK/KZG
// commit path"; the reference has no GPU path for PLONK, SURVEY.md §0.2).
//
// Seams in backend/plonk/bls12-377/prove.go, all behind the same
// backend.WithIcicleAcceleration() option (ProverConfig.Accelerator == "icicle"):
//
//  1. Every n-size MSM.  kzg.Commit(p, pk.KzgLagrange) at prove.go:312, 460 ->
//     commitLagrange; kzg.Commit(p, pk.Kzg) at :718 and the three quotient
//     commitments of commitToQuotient (:1154-1170) -> commitCanonical; the
//     opening quotients of kzg.Open (:611) and kzg.BatchOpenSinglePoint (:757)
//     -> open / batchOpen: the polynomials are uploaded once; the claimed
//     values, the fold sum_i gamma^i f_i and the division by X - z run on the
//     device (gm_kzg_eval, gm_kzg_open, gm_kzg_batch_open: the same canonical Fr
//     bytes as gnark-crypto's Horner evaluation and dividePolyByXminusA,
//     tests/test_kzg_open_gpu.py), and the quotient goes from device memory
//     straight into the MSM over the SRS kept resident (same digest bytes as
//     kzg.Commit, tests/test_msm_gpu.py::test_kzg_commit_and_prepared_msm).
//     Only gamma is derived on the host, between the two device steps.  The SRS
//     is selected explicitly by the caller, never by pointer identity.
//     The quotient stage as one device call (gm_plonk_quotient, resident
//     polynomials in, h out) -> quotient; computeQuotient does not call it yet.
//     The copy-constraint accumulator Z as one device call (gm_plonk_perm_z:
//     ratios, scan, one inversion) with its commitment over the Lagrange SRS read
//     where Z lies -> ratioZ; buildRatioCopyConstraint (:565-597) does not call it
//     yet.
//     The linearized polynomial as one device call (gm_plonk_linearize: the
//     evaluations at zeta, one streaming combination) with its commitment read
//     where it lies -> linearize; computeLinearizedPolynomial (:656-724) does not
//     call it yet.
//  2. Every n- and 4n-size FFT.  The domain0 ToCanonical / ToLagrange of
//     computeNumerator (:949, :967, :1016) and of computeLinearizedPolynomial
//     (:1301) -> toCanonical / toLagrange, and divideByZH's domain1 coset
//     FFTInverse (:1201) -> fftDomain1: gm.NTT with iop's decimation choice
//     (Regular -> DIF, BitReverse -> DIT: the layout flips, no bit reversal).
//
// Parity: the commits and transforms are replayed call for call against the
// oracle in tests/test_plonk_replay_gpu.py.  batchOpen's Fiat-Shamir challenge
// restates gnark-crypto's unexported kzg.deriveGamma (transcript "gamma":
// point, digests, claimed values, data); it cannot be compiled or run here (no
// Go toolchain), so every GPU batch opening is checked with gnark-crypto's own
// kzg.BatchVerifySinglePoint before it is used, and the CPU
// kzg.BatchOpenSinglePoint runs instead if the check fails.
//
// Wiring: prove.go.diff in this directory (a real patch against the
// reference's backend/plonk/bls12-377/prove.go; INTEGRATION.md §5).
// Without the icicle tag kzg_mi355x_stub.go keeps the patched file compiling
// (deviceFor returns nil and every call stays on gnark-crypto).
//
// NOT COMPILED HERE: this image has no Go toolchain.
package plonk

import (
	"errors"
	"hash"
	"os"
	"sync"
	"unsafe"

	curve "github.com/consensys/gnark-crypto/ecc/bls12-377"
	"github.com/consensys/gnark-crypto/ecc/bls12-377/fr"
	"github.com/consensys/gnark-crypto/ecc/bls12-377/fr/fft"
	"github.com/consensys/gnark-crypto/ecc/bls12-377/fr/iop"
	"github.com/consensys/gnark-crypto/ecc/bls12-377/kzg"
	fiatshamir "github.com/consensys/gnark-crypto/fiat-shamir"

	"github.com/consensys/gnark/backend/accel/mi355x/gm"
)

// kzgDevice keeps pk.Kzg.G1 and pk.KzgLagrange.G1 resident on the GPU (uploaded
// once per proving key, like setupDevicePointers does for Groth16).
type kzgDevice struct {
	once            sync.Once
	canonical, lagr *gm.SRS
	nCanon, nLagr   int
	vk              kzg.VerifyingKey
	err             error
}

// one kzgDevice per proving key (the SRS is uploaded once per key)
var devices sync.Map // *ProvingKey -> *kzgDevice

// deviceFor returns pk's device state, uploading its SRS on first use; nil when
// no GPU is usable (the prover then stays on the CPU path).
func deviceFor(pk *ProvingKey) *kzgDevice {
	v, _ := devices.LoadOrStore(pk, &kzgDevice{})
	d := v.(*kzgDevice)
	if d.setup(pk) != nil {
		return nil
	}
	return d
}

func (d *kzgDevice) setup(pk *ProvingKey) error {
	d.once.Do(func() {
		if len(pk.Kzg.G1) == 0 || len(pk.KzgLagrange.G1) == 0 || pk.Vk == nil {
			d.err = errors.New("gnark_mi355x: proving key without an SRS")
			return
		}
		if d.canonical, d.err = gm.UploadSRS(gm.BLS12_377, unsafe.Pointer(&pk.Kzg.G1[0]), len(pk.Kzg.G1)); d.err != nil {
			return
		}
		if d.lagr, d.err = gm.UploadSRS(gm.BLS12_377, unsafe.Pointer(&pk.KzgLagrange.G1[0]), len(pk.KzgLagrange.G1)); d.err != nil {
			return
		}
		d.nCanon, d.nLagr = len(pk.Kzg.G1), len(pk.KzgLagrange.G1)
		d.vk = pk.Vk.Kzg
	})
	return d.err
}

// commitWith replaces kzg.Commit(p, key) for the resident SRS srs of nSRS
// points: kzg.ErrInvalidPolynomialSize when p is longer, else the G1 digest
// sum_i p[i] * key.G1[i].
func commitWith(srs *gm.SRS, nSRS int, p []fr.Element) (kzg.Digest, error) {
	if len(p) > nSRS {
		return kzg.Digest{}, kzg.ErrInvalidPolynomialSize
	}
	var out curve.G1Affine
	if len(p) == 0 {
		return out, nil
	}
	if err := srs.Commit(unsafe.Pointer(&p[0]), len(p), unsafe.Pointer(&out)); err != nil {
		return kzg.Digest{}, err
	}
	return out, nil
}

// commitLagrange: kzg.Commit(p, pk.KzgLagrange) (p in Lagrange form).
func (d *kzgDevice) commitLagrange(p []fr.Element) (kzg.Digest, error) {
	return commitWith(d.lagr, d.nLagr, p)
}

// commitCanonical: kzg.Commit(p, pk.Kzg) (p in canonical form).
func (d *kzgDevice) commitCanonical(p []fr.Element) (kzg.Digest, error) {
	return commitWith(d.canonical, d.nCanon, p)
}

// open replaces kzg.Open(p, z, pk.Kzg) (prove.go:611): p is uploaded once, the
// claimed value p(z) and the quotient (p - p(z)) / (X - z) are formed on the
// device (gm_kzg_open) and the quotient goes straight into the MSM.  The
// quotient is unique and Fr results are canonical, so H is kzg.Open's byte for
// byte.
func (d *kzgDevice) open(p []fr.Element, z fr.Element) (kzg.OpeningProof, error) {
	if len(p) == 0 || len(p) > d.nCanon {
		return kzg.OpeningProof{}, kzg.ErrInvalidPolynomialSize
	}
	dp, err := gm.UploadPoly(unsafe.Pointer(&p[0]), len(p))
	if err != nil {
		return kzg.OpeningProof{}, err
	}
	defer dp.Free()
	var res kzg.OpeningProof
	if err := d.canonical.Open(dp, unsafe.Pointer(&z), unsafe.Pointer(&res.ClaimedValue),
		unsafe.Pointer(&res.H)); err != nil {
		return kzg.OpeningProof{}, err
	}
	return res, nil
}

// deriveGamma restates gnark-crypto kzg's transcript for folding: challenge
// "gamma" bound to the point, the digests, the claimed values and the extra
// transcript data, in that order.
func deriveGamma(z fr.Element, digests []kzg.Digest, claimed []fr.Element, hf hash.Hash,
	data ...[]byte) (fr.Element, error) {
	fs := fiatshamir.NewTranscript(hf, "gamma")
	if err := fs.Bind("gamma", z.Marshal()); err != nil {
		return fr.Element{}, err
	}
	for i := range digests {
		if err := fs.Bind("gamma", digests[i].Marshal()); err != nil {
			return fr.Element{}, err
		}
	}
	for i := range claimed {
		if err := fs.Bind("gamma", claimed[i].Marshal()); err != nil {
			return fr.Element{}, err
		}
	}
	for i := range data {
		if err := fs.Bind("gamma", data[i]); err != nil {
			return fr.Element{}, err
		}
	}
	b, err := fs.ComputeChallenge("gamma")
	if err != nil {
		return fr.Element{}, err
	}
	var gamma fr.Element
	gamma.SetBytes(b)
	return gamma, nil
}

var errBatchCheck = errors.New("gnark_mi355x: GPU batch opening failed its verification")

// batchOpen replaces kzg.BatchOpenSinglePoint(polys, digests, z, hf, pk.Kzg,
// data...) (prove.go:757).  The polynomials are uploaded once and stay on the
// device for both steps: the claimed values f_i(z) (gm_kzg_eval), then -- gamma
// depends on them, so it is derived on the host in between -- the fold
// F = sum_i gamma^i f_i, its quotient (F - F(z)) / (X - z) and the commitment
// (gm_kzg_batch_open).  The result is checked with kzg.BatchVerifySinglePoint
// (gnark-crypto's own transcript); errBatchCheck tells the caller to use the
// CPU opening instead.
func (d *kzgDevice) batchOpen(polys [][]fr.Element, digests []kzg.Digest, z fr.Element, hf hash.Hash,
	data ...[]byte) (kzg.BatchOpeningProof, error) {
	if len(polys) != len(digests) || len(polys) == 0 {
		return kzg.BatchOpeningProof{}, kzg.ErrInvalidNbDigests
	}
	largest := 0
	for i := range polys {
		if len(polys[i]) > d.nCanon {
			return kzg.BatchOpeningProof{}, kzg.ErrInvalidPolynomialSize
		}
		if len(polys[i]) > largest {
			largest = len(polys[i])
		}
	}
	if largest == 0 {
		return kzg.BatchOpeningProof{}, errBatchCheck
	}
	devs := make([]*gm.DevicePoly, len(polys))
	defer func() {
		for _, dp := range devs {
			dp.Free()
		}
	}()
	var err error
	for i := range polys {
		var src unsafe.Pointer
		if len(polys[i]) > 0 {
			src = unsafe.Pointer(&polys[i][0])
		}
		if devs[i], err = gm.UploadPoly(src, len(polys[i])); err != nil {
			return kzg.BatchOpeningProof{}, err
		}
	}
	var res kzg.BatchOpeningProof
	res.ClaimedValues = make([]fr.Element, len(polys))
	if err = gm.EvalPolys(gm.BLS12_377, devs, unsafe.Pointer(&z), unsafe.Pointer(&res.ClaimedValues[0])); err != nil {
		return kzg.BatchOpeningProof{}, err
	}
	hf.Reset()
	gamma, err := deriveGamma(z, digests, res.ClaimedValues, hf, data...)
	if err != nil {
		return kzg.BatchOpeningProof{}, err
	}
	if err = d.canonical.BatchOpen(devs, unsafe.Pointer(&z), unsafe.Pointer(&gamma), nil,
		unsafe.Pointer(&res.H)); err != nil {
		return kzg.BatchOpeningProof{}, err
	}
	hf.Reset()
	if err := kzg.BatchVerifySinglePoint(digests, &res, z, hf, d.vk, data...); err != nil {
		return kzg.BatchOpeningProof{}, errBatchCheck
	}
	hf.Reset()
	return res, nil
}

// quotientPolys orders the fixed inputs of quotient: the selectors, the
// permutation polynomials, the wires and Z.
const (
	qQl = iota
	qQr
	qQm
	qQo
	qQk
	qS1
	qS2
	qS3
	qL
	qR
	qO
	qZ
)

const quotientPolys = 12

var errQuotientShape = errors.New("gnark_mi355x: quotient inputs of the wrong size")

// quotient runs computeNumerator + divideByZH (prove.go:771-1034, :1178-1231)
// as one device call (gm_plonk_quotient).  polys and the BSB22 pairs qcp / pi2
// are canonical, regular polynomials of n coefficients, l, r, o and z NOT
// blinded; bl, br, bo (2 coefficients) and bz (3) are the blinding polynomials.
// Returns h1, h2, h3 (n + 2 coefficients each), the slices commitToQuotient
// commits.  StatisticalZK's randomisation of them stays with the caller.  n < 8
// (the reference's 8n domain) is refused: the caller keeps the CPU path.
//
// Not yet called from computeQuotient: prove.go.diff still takes the stage one
// transform at a time.
func (d *kzgDevice) quotient(n int, polys [quotientPolys][]fr.Element, qcp, pi2 [][]fr.Element,
	bl, br, bo, bz []fr.Element, alpha, beta, gamma fr.Element) ([3][]fr.Element, error) {
	var res [3][]fr.Element
	if n < 8 || len(qcp) != len(pi2) || len(bl) != 2 || len(br) != 2 || len(bo) != 2 || len(bz) != 3 {
		return res, errQuotientShape
	}
	var devs []*gm.DevicePoly
	defer func() {
		for _, dp := range devs {
			dp.Free()
		}
	}()
	upload := func(p []fr.Element) (*gm.DevicePoly, error) {
		if len(p) != n {
			return nil, errQuotientShape
		}
		dp, err := gm.UploadPoly(unsafe.Pointer(&p[0]), n)
		if err == nil {
			devs = append(devs, dp)
		}
		return dp, err
	}
	var fixed [quotientPolys]*gm.DevicePoly
	var err error
	for i := range polys {
		if fixed[i], err = upload(polys[i]); err != nil {
			return res, err
		}
	}
	in := gm.QuotientInput{
		N:  n,
		Ql: fixed[qQl], Qr: fixed[qQr], Qm: fixed[qQm], Qo: fixed[qQo], Qk: fixed[qQk],
		S1: fixed[qS1], S2: fixed[qS2], S3: fixed[qS3],
		L: fixed[qL], R: fixed[qR], O: fixed[qO], Z: fixed[qZ],
		Bl: unsafe.Pointer(&bl[0]), Br: unsafe.Pointer(&br[0]), Bo: unsafe.Pointer(&bo[0]), Bz: unsafe.Pointer(&bz[0]),
		Alpha: unsafe.Pointer(&alpha), Beta: unsafe.Pointer(&beta), Gamma: unsafe.Pointer(&gamma),
	}
	for i := range qcp {
		var a, b *gm.DevicePoly
		if a, err = upload(qcp[i]); err != nil {
			return res, err
		}
		if b, err = upload(pi2[i]); err != nil {
			return res, err
		}
		in.Qcp, in.Pi2 = append(in.Qcp, a), append(in.Pi2, b)
	}
	h, err := gm.AllocPoly(4 * n)
	if err != nil {
		return res, err
	}
	devs = append(devs, h)
	if err = gm.PlonkQuotient(gm.BLS12_377, &in, h); err != nil {
		return res, err
	}
	for i := range res {
		res[i] = make([]fr.Element, n+2)
		if err = h.Download(unsafe.Pointer(&res[i][0]), i*(n+2), n+2); err != nil {
			return [3][]fr.Element{}, err
		}
	}
	return res, nil
}

var errRatioShape = errors.New("gnark_mi355x: permutation inputs of the wrong size")

// ratioZ runs buildRatioCopyConstraint (prove.go:565-597: iop's
// BuildRatioCopyConstraint and the commitment of Z over the Lagrange SRS) as one
// device call and one MSM on the resident result (gm_plonk_perm_z,
// gm_msm_prepared).  l, r, o are the solved wires and s1, s2, s3 the trace's
// permutation polynomials, all n values in Lagrange basis, regular order.  Returns
// Z in Lagrange form, Z in canonical form (not blinded: the z of quotient) and the
// commitment of the Lagrange form.  n < 8 is refused: the caller keeps the CPU
// path.
//
// Not yet called from buildRatioCopyConstraint: prove.go.diff still builds Z
// with iop on the host.
func (d *kzgDevice) ratioZ(n int, l, r, o, s1, s2, s3 []fr.Element, beta, gamma fr.Element) ([]fr.Element,
	[]fr.Element, kzg.Digest, error) {
	if n < 8 || n > d.nLagr {
		return nil, nil, kzg.Digest{}, errRatioShape
	}
	var devs []*gm.DevicePoly
	defer func() {
		for _, dp := range devs {
			dp.Free()
		}
	}()
	var in [6]*gm.DevicePoly
	for i, p := range [6][]fr.Element{l, r, o, s1, s2, s3} {
		if len(p) != n {
			return nil, nil, kzg.Digest{}, errRatioShape
		}
		dp, err := gm.UploadPoly(unsafe.Pointer(&p[0]), n)
		if err != nil {
			return nil, nil, kzg.Digest{}, err
		}
		devs = append(devs, dp)
		in[i] = dp
	}
	var out [2]*gm.DevicePoly
	for i := range out {
		dp, err := gm.AllocPoly(n)
		if err != nil {
			return nil, nil, kzg.Digest{}, err
		}
		devs = append(devs, dp)
		out[i] = dp
	}
	perm := gm.PermInput{
		N: n,
		L: in[0], R: in[1], O: in[2], S1: in[3], S2: in[4], S3: in[5],
		Beta: unsafe.Pointer(&beta), Gamma: unsafe.Pointer(&gamma),
	}
	if err := gm.PlonkPermZ(gm.BLS12_377, &perm, out[0], out[1]); err != nil {
		return nil, nil, kzg.Digest{}, err
	}
	var digest curve.G1Affine
	if err := d.lagr.CommitResident(out[0], 0, n, unsafe.Pointer(&digest)); err != nil {
		return nil, nil, kzg.Digest{}, err
	}
	zl, zc := make([]fr.Element, n), make([]fr.Element, n)
	if err := out[0].Download(unsafe.Pointer(&zl[0]), 0, n); err != nil {
		return nil, nil, kzg.Digest{}, err
	}
	if err := out[1].Download(unsafe.Pointer(&zc[0]), 0, n); err != nil {
		return nil, nil, kzg.Digest{}, err
	}
	return zl, zc, digest, nil
}

var errLinearizeShape = errors.New("gnark_mi355x: linearization inputs of the wrong size")

// linearize runs computeLinearizedPolynomial (prove.go:656-724: the evaluations
// at zeta, innerComputeLinearizedPoly and the commitment of its result) as one
// device call and one MSM on the resident result (gm_plonk_linearize,
// gm_msm_prepared).  polys, qcp, pi2 and the blinding polynomials are quotient's
// (l, r, o, z NOT blinded, Qk completed); h holds the 4n coefficients of the
// quotient, of which the first 3 (n + 2) are read; hRand is nil or
// StatisticalZK's two shard randomizers.  Returns the linearized polynomial
// (n + 3 coefficients), its commitment over the canonical SRS and the evaluations
// l~(zeta), r~(zeta), o~(zeta), s1(zeta), s2(zeta), z~(w zeta), qcp_j(zeta).  n < 8
// is refused: the caller keeps the CPU path.
//
// Not yet called from computeLinearizedPolynomial: prove.go.diff still builds the
// polynomial on the host and commits it with commitCanonical.
func (d *kzgDevice) linearize(n int, polys [quotientPolys][]fr.Element, qcp, pi2 [][]fr.Element,
	bl, br, bo, bz, h, hRand []fr.Element, alpha, beta, gamma, zeta fr.Element) ([]fr.Element, kzg.Digest,
	[]fr.Element, error) {
	if n < 8 || n+3 > d.nCanon || len(qcp) != len(pi2) || len(bl) != 2 || len(br) != 2 || len(bo) != 2 ||
		len(bz) != 3 || len(h) != 4*n || (hRand != nil && len(hRand) != 2) {
		return nil, kzg.Digest{}, nil, errLinearizeShape
	}
	var devs []*gm.DevicePoly
	defer func() {
		for _, dp := range devs {
			dp.Free()
		}
	}()
	upload := func(p []fr.Element, size int) (*gm.DevicePoly, error) {
		if len(p) != size {
			return nil, errLinearizeShape
		}
		dp, err := gm.UploadPoly(unsafe.Pointer(&p[0]), size)
		if err == nil {
			devs = append(devs, dp)
		}
		return dp, err
	}
	var fixed [quotientPolys]*gm.DevicePoly
	var err error
	for i := range polys {
		if fixed[i], err = upload(polys[i], n); err != nil {
			return nil, kzg.Digest{}, nil, err
		}
	}
	in := gm.LinearizeInput{
		N:  n,
		Ql: fixed[qQl], Qr: fixed[qQr], Qm: fixed[qQm], Qo: fixed[qQo], Qk: fixed[qQk],
		S1: fixed[qS1], S2: fixed[qS2], S3: fixed[qS3],
		L: fixed[qL], R: fixed[qR], O: fixed[qO], Z: fixed[qZ],
		Bl: unsafe.Pointer(&bl[0]), Br: unsafe.Pointer(&br[0]), Bo: unsafe.Pointer(&bo[0]), Bz: unsafe.Pointer(&bz[0]),
		Alpha: unsafe.Pointer(&alpha), Beta: unsafe.Pointer(&beta), Gamma: unsafe.Pointer(&gamma),
		Zeta: unsafe.Pointer(&zeta),
	}
	if hRand != nil {
		in.HRand = unsafe.Pointer(&hRand[0])
	}
	for i := range qcp {
		var a, b *gm.DevicePoly
		if a, err = upload(qcp[i], n); err != nil {
			return nil, kzg.Digest{}, nil, err
		}
		if b, err = upload(pi2[i], n); err != nil {
			return nil, kzg.Digest{}, nil, err
		}
		in.Qcp, in.Pi2 = append(in.Qcp, a), append(in.Pi2, b)
	}
	if in.H, err = upload(h, 4*n); err != nil {
		return nil, kzg.Digest{}, nil, err
	}
	lin, err := gm.AllocPoly(n + 3)
	if err != nil {
		return nil, kzg.Digest{}, nil, err
	}
	devs = append(devs, lin)
	evals := make([]fr.Element, 6+len(qcp))
	out := gm.LinearizeOutput{Lin: lin, Evals: unsafe.Pointer(&evals[0])}
	if err = gm.PlonkLinearize(gm.BLS12_377, &in, &out); err != nil {
		return nil, kzg.Digest{}, nil, err
	}
	var digest curve.G1Affine
	if err = d.canonical.CommitResident(lin, 0, n+3, unsafe.Pointer(&digest)); err != nil {
		return nil, kzg.Digest{}, nil, err
	}
	res := make([]fr.Element, n+3)
	if err = lin.Download(unsafe.Pointer(&res[0]), 0, n+3); err != nil {
		return nil, kzg.Digest{}, nil, err
	}
	return res, digest, evals, nil
}

// plainForm: a Lagrange or Canonical (not coset) polynomial of |dom|
// coefficients -- the only inputs the GPU transforms take; anything else
// (already in the target basis, coset forms, other sizes) goes to iop.
func plainForm(p *iop.Polynomial, dom *fft.Domain, from iop.Basis) bool {
	return p != nil && p.Basis == from && len(p.Coefficients()) == int(dom.Cardinality) &&
		os.Getenv("GNARK_MI355X_PLONK_FFT") != "0"
}

// toCanonical runs p.ToCanonical(dom) for a Lagrange p on the GPU: FFTInverse
// DIF on a Regular layout, DIT on a BitReverse one, and the layout flips (iop's
// choice: no bit-reversal pass).  false: the caller runs iop's transform.
func (d *kzgDevice) toCanonical(p *iop.Polynomial, dom *fft.Domain) bool {
	if !plainForm(p, dom, iop.Lagrange) {
		return false
	}
	c := p.Coefficients()
	dit := p.Layout == iop.BitReverse
	if gm.NTT(gm.BLS12_377, unsafe.Pointer(&c[0]), len(c), true, dit, false) != nil {
		return false
	}
	p.Basis = iop.Canonical
	p.Layout = flip(p.Layout)
	return true
}

// toLagrange: p.ToLagrange(dom) for a Canonical p (FFT, DIF / DIT as above).
func (d *kzgDevice) toLagrange(p *iop.Polynomial, dom *fft.Domain) bool {
	if !plainForm(p, dom, iop.Canonical) {
		return false
	}
	c := p.Coefficients()
	dit := p.Layout == iop.BitReverse
	if gm.NTT(gm.BLS12_377, unsafe.Pointer(&c[0]), len(c), false, dit, false) != nil {
		return false
	}
	p.Basis = iop.Lagrange
	p.Layout = flip(p.Layout)
	return true
}

func flip(l iop.Layout) iop.Layout {
	if l == iop.Regular {
		return iop.BitReverse
	}
	return iop.Regular
}

// fftDomain1 runs the domain1 transform of prove.go's quotient on the GPU:
// inverse selects FFTInverse, dit the DIT decimation, coset fft.OnCoset()
// (divideByZH: FFTInverse(DIT, OnCoset), bit-reversed in, natural out).
func (d *kzgDevice) fftDomain1(v []fr.Element, inverse, dit, coset bool) error {
	if len(v) == 0 {
		return nil
	}
	return gm.NTT(gm.BLS12_377, unsafe.Pointer(&v[0]), len(v), inverse, dit, coset)
}

"""Non-R driver of the AM() forward-selection loop -- host side, numpy/LAPACK.

This is the reference's model loop restated so that "the same SNPs are selected" can be demonstrated end to end on
a box without R: constructX -> calcMMt (GPU) -> emma.REMLE -> extBIC via emma.MLE -> find_qtl (GPU scan + arg-max).
Everything n x n stays on the host by design (north_star keeps emma_REMLE / calculateP / calculateH on host LAPACK);
the two marker-dimension operations go through a `backend` whose default is the HIP library (r_api).

Reference lines (E/ = MyPackage/Eagle/):
  AM loop ........................ E/R/AM.R:400-475 (stop rule :448, maxit :463)
  .calcVC ........................ E/R/calcVC.R:1-8           emma.REMLE  E/R/emma_REMLE.R:27-131
  .calc_extBIC ................... E/R/calc_extBIC.R:1-12     emma.MLE    E/R/emma_MLE.R:2-117
  emma.eigen.R.wo.Z / L.wo.Z ..... E/R/emma_eigen_R_wo_Z.R:2-21, E/R/emma_eigen_L_wo_Z.R:1-12
  constructX / extract_geno ...... E/R/constructX.R:1-24, E/R/extract_geno.R:1-19

With a Z matrix (AM(Zmat=), repeated measures) the variance components and extBIC restate the reference's emma_*_w_Z path in a
reduced t x t form; its own .find_qtl takes no Z and fails (SURVEY.md section 8a, config 5 note), so the scan of that model is this
project's definition.
parity unpinned: the reference records no outputs, and R's uniroot (Brent, tol = eps^0.25) is restated from the
published zeroin algorithm, not from R's source.
"""
import math

import numpy as np
from scipy.special import chdtr, gammaln

from . import host_model
from .emma import (_EPS25, _emma_eig, _emma_eig_batch, _emma_result, _emma_z, _eig_grid_dll, _eig_grid_dll_batch,  # noqa: F401
                   _grid, _grid_memo, _grid_weights, _ml_dll, _ml_ll, _optimise, _optimum, _reml_dll, _reml_ll, _z_dll, _z_fit, _z_ll,
                   _zeroin, as_ind_of_obs, emma_eigen_L_wo_Z, emma_eigen_R_wo_Z, emma_MLE, emma_MLE_eig, emma_MLE_eig_batch,
                   emma_REMLE, emma_REMLE_eig, emma_REMLE_eig_batch)   # all of emma stays reachable as am.<name>


def calcVC(trait, currentX, MMt, eig_R=None, Z=None, zmodel=None, eig_L=None):
    """eig_L is not used: it is taken so that one set of keywords serves calcVC and calc_extBIC."""
    r = emma_REMLE(trait, currentX, MMt, Z=Z, eig_R=eig_R, zmodel=zmodel)
    return {k: r[k] for k in ("vg", "ve")}


def _lchoose(n, k):
    return gammaln(n + 1) - gammaln(k + 1) - gammaln(n - k + 1)


def _extBIC(ML, k, n, nmarkers, gamma):
    """calc_extBIC.R:7-9 for a model of k fixed-effect columns on n records, gamma weighting the model-space term."""
    return -2 * ML + (k + 1) * math.log(n) + 2 * gamma * _lchoose(nmarkers, k - 1)


def calc_extBIC(trait, currentX, MMt, nmarkers, eig_L=None, eig_R=None, Z=None, zmodel=None, gamma=1.0):
    """calc_extBIC.R:1-12 with the weight gamma on the model-space term; gamma = 1 is the reference's
    value bit for bit, 2 * 1.0 being exact."""
    res = emma_MLE(trait, currentX, MMt, Z=Z, llim=-100, ulim=100, eig_L=eig_L, eig_R=eig_R, zmodel=zmodel)
    return _extBIC(res["ML"], currentX.shape[1], trait.size, nmarkers, gamma)


class HipBackend:
    """The two marker-dimension calls of the loop on the GPU (r_api mirrors the R wrappers' marshalling)."""

    def __init__(self, device=0):
        from . import r_api, rcpp_api
        self.r_api, self.rcpp_api, self.device = r_api, rcpp_api, device

    def calcMMt(self, geno, availmemGb, ncpu, selected_loci, quiet):
        return self.r_api.calcMMt(geno, availmemGb, ncpu, selected_loci, quiet, device=self.device)

    def find_qtl(self, **kw):
        return self.r_api.find_qtl(device=self.device, **kw)

    def extract_geno(self, geno, colnum):
        """extract_geno.R:8-12: column colnum (1-based) of M.ascii, served from the HBM-resident copy calcMMt left."""
        return self.r_api.extract_geno(geno["asciifileM"], colnum, dim_of_ascii_M=geno["dim_of_ascii_M"],
                                       device=self.device).astype(np.int64)

    def reshape(self, geno, indxNA):
        """AM.R:345-366 in VIEW mode: drops the individuals indxNA (1-based) from both genotype files without writing either; the
        returned geno names the views."""
        return reshape_geno(geno, indxNA, view=True, device=self.device)


class SpectralBackend(HipBackend):
    """The same loop with the scan in the eigenbasis of MM^T (include/eagle_hip.h section 1d; OPT-IN, needs the R-side change
    INTEGRATION.md describes): K = MM^T/max + 0.95 I is fixed for the whole run, so Z = Mt U is made once after calcMMt and
    every find_qtl is one HBM-bound pass over Z instead of an n x n quadratic form per marker.  Selects the markers the
    reference-shaped path selects (tests/test_am_driver.py)."""

    def __init__(self, device=0):
        super().__init__(device)
        self.lam = self.U = None
        self.L = None

    calcMMt_plain = HipBackend.calcMMt    # K alone: what AM(Zmat=) asks for, followed by prepare_z

    def prepare_z(self, geno, zmodel, availmemGb):
        """Repeated measures: Z~ = Mt (D^1/2 U~ / sqrt(d_max)) for U~ of D^1/2 K D^1/2 (host_model.ZModel), once per run."""
        self.lam = self.U = None
        n, self.L = geno["dim_of_ascii_M"]
        basis, _ = zmodel.spectral_basis()
        self.rcpp_api.spectral_prepare(geno["asciifileMt"], (self.L, n), basis, availmemGb, device=self.device)

    def calcMMt(self, geno, availmemGb, ncpu, selected_loci, quiet):
        MMt = super().calcMMt(geno, availmemGb, ncpu, selected_loci, quiet)
        self.lam, self.U = np.linalg.eigh(MMt)                       # the decomposition emma.REMLE needs anyway
        n, self.L = geno["dim_of_ascii_M"]
        self.rcpp_api.spectral_prepare(geno["asciifileMt"], (self.L, n), self.U, availmemGb, device=self.device)
        return MMt

    @property
    def eig(self):
        """(lam, U) of the last run's K, what r_api.SummaryAM(..., eig=) takes instead of its own eigh; None before a run."""
        return None if self.U is None else (self.lam, self.U)

    def find_qtl(self, geno, availmemGb, selected_loci, MMt, invMMt, best_ve, best_vg, currentX, ncpu, quiet, trait, Zmat=None):
        if Zmat is not None:   # a host_model.ZModel whose basis prepare_z made resident
            op = Zmat.spectral_operands(currentX, trait, best_ve, best_vg)
            res = self.rcpp_api.spectral_scan_weights(op["d"], op["Gy"], op["GX"], op["C"], op["c1"], best_vg, self.L, selected_loci,
                                                      device=self.device)
        else:
            res = self.rcpp_api.spectral_scan(self.lam, self.U.T @ currentX, self.U.T @ np.ravel(trait), best_ve, best_vg, self.L,
                                              selected_loci, device=self.device)
        with np.errstate(all="ignore"):
            tsq = res["a"].ravel() ** 2 / res["vara"].ravel()
        return int(np.flatnonzero(tsq == np.nanmax(tsq))[0]) + 1         # find_qtl.R:71-83


def reshape_geno(geno, indxNA, view=False, device=0):
    """AM.R:345-366: ReshapeM on the two files of `geno`, then geno names the results (<file>tmp) and carries the new dims.
    view=False writes the files (what a backend without its own `reshape` gets); view=True registers views on `device`."""
    from . import r_api
    newdims = r_api.ReshapeM(geno["asciifileM"], geno["asciifileMt"], indxNA, geno["dim_of_ascii_M"], view=view, device=device)
    return {"asciifileM": geno["asciifileM"] + "tmp", "asciifileMt": geno["asciifileMt"] + "tmp", "dim_of_ascii_M": newdims}


def add_pcs(X, pca, k=None):
    """X with the first k (default all) columns of r_api.PCA()'s "pcs" appended: the design matrix of AM(trait, X, geno) with
    principal components as fixed effects (the reference's documented fformula = "pc1 + pc2").  X and pcs must hold the same
    individuals, in the order of the panel."""
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(-1, 1) if X.ndim == 1 else X
    pcs = np.asarray(pca["pcs"], dtype=np.float64)
    k = pcs.shape[1] if k is None else int(k)
    if k < 0 or k > pcs.shape[1]:
        raise ValueError("add_pcs: k = %d of %d components" % (k, pcs.shape[1]))
    if X.shape[0] != pcs.shape[0]:
        raise ValueError("add_pcs: X holds %d individuals, the components %d" % (X.shape[0], pcs.shape[0]))
    return np.concatenate([X, pcs[:, :k]], axis=1)


def add_ancestry(X, adm):
    """X with the first K - 1 columns of r_api.Admixture()'s "Q" appended: ancestry fractions as fixed effects of AM, GWAS or Logistic,
    the model-based twin of add_pcs.  The last column is left out: the rows of Q sum to 1, so it is collinear with the intercept.  X
    and Q must hold the same individuals, in the order of the panel."""
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(-1, 1) if X.ndim == 1 else X
    Q = np.asarray(adm["Q"], dtype=np.float64)
    if Q.ndim != 2 or X.shape[0] != Q.shape[0]:
        raise ValueError("add_ancestry: X holds %d individuals, Q %s" % (X.shape[0], Q.shape[:1]))
    return np.concatenate([X, Q[:, :Q.shape[1] - 1]], axis=1)


def _reshape(geno, indxNA, backend=None, device=0):
    """geno without the individuals indxNA: backend.reshape, reshape_geno writing the files for a backend without one, or for a
    caller that has no backend a view on `device`."""
    if backend is None:
        return reshape_geno(geno, indxNA, view=True, device=device)
    return backend.reshape(geno, indxNA) if hasattr(backend, "reshape") else reshape_geno(geno, indxNA)


def _drop_na_rows(indxNA, arrays, geno=None, say=None, backend=None, device=0):
    """AM.R:337-366: the rows indxNA (1-based) leave every one of `arrays`, `say` is told so, and a `geno` is reshaped (_reshape).
    -> the arrays, geno.  Nothing happens for an empty indxNA."""
    if not indxNA.size:
        return arrays, geno
    keep = np.ones(arrays[0].shape[0], dtype=bool)
    keep[indxNA - 1] = False
    if say is not None:
        say(" The following rows are being removed from pheno due to missing data: %s" % " ".join(str(int(i)) for i in indxNA))
    return [a[keep] for a in arrays], geno if geno is None else _reshape(geno, indxNA, backend, device)


# ---------------------------------------------------------------------------------------------------------------------------
# The forward-selection loop (AM.R:400-499), its rules stated once for AM() with and without Zmat and for AM_traits: a run's
# state is a dict of sel (the picks after the leading NA of AM.R:260), ext (the extBIC trace), best (the last ve, vg), itnum, cont.
# ---------------------------------------------------------------------------------------------------------------------------
def _loop_state(**more):
    return dict({"sel": [np.nan], "ext": [], "best": {}, "itnum": 1, "cont": True}, **more)


def _still_improving(extBIC):
    """AM.R:448: the search goes on while the newest extBIC is the first minimum of the trace."""
    return int(np.flatnonzero(np.asarray(extBIC) == min(extBIC))[0]) == len(extBIC) - 1


def _end_iteration(s, maxit):
    s["itnum"] += 1
    if s["itnum"] > maxit:  # AM.R:463-470
        s["cont"] = False


def _AM_result(s, maxit, indxNA, geno):
    """AM.R:476-499.  Stopped by maxit: every pick is reported (the in-loop report that drops the last pick is overwritten by
    the one after the loop).  Stopped by extBIC: the last pick made extBIC worse and is dropped together with its extBIC entry."""
    picks = [int(v) for v in s["sel"][1:]]
    if s["itnum"] > maxit or len(s["sel"]) <= 1:
        loci, ext = picks, list(s["ext"])
    else:
        loci = picks[:-1]
        ext = [v for i, v in enumerate(s["ext"]) if i != len(s["sel"]) - 1]
    return {"selected_loci": loci, "all_picks": picks, "extBIC": ext, "extBIC_trace": list(s["ext"]), "ve": s["best"].get("ve"),
            "vg": s["best"].get("vg"), "indxNA": indxNA, "dim_of_ascii_M": list(geno["dim_of_ascii_M"])}


def _plain_model(backend):
    """Where AM()'s loop depends on the model, for one record per individual -> prepare (the first iteration, AM.R:414-422; returns
    MMt), fit_kw (X -> what calcVC and calc_extBIC of one iteration share), column (a marker column as it enters X), scan_kw (the
    model's keywords of find_qtl)."""
    k = {}

    def prepare(geno, *args):
        k["MMt"] = backend.calcMMt(geno, *args)
        k["invMMt"] = host_model._chol2inv(k["MMt"])
        k["eig_L"] = emma_eigen_L_wo_Z(k["MMt"])  # depends on MMt only; the reference recomputes it every iteration
        return k["MMt"]

    return (prepare, lambda X: {"eig_L": k["eig_L"], "eig_R": emma_eigen_R_wo_Z(k["MMt"], X)}, lambda m: m,
            lambda: {"invMMt": k["invMMt"]})


def _z_model(backend, ind):
    """_plain_model for AM(Zmat=), ind = ind_of_obs: K alone, then the one eigh of the run (ZModel) and the backend's Z build; a marker
    enters X as Z m_j."""
    k = {}

    def prepare(geno, availmemGb, *args):
        MMt = getattr(backend, "calcMMt_plain", backend.calcMMt)(geno, availmemGb, *args)
        k["zm"] = host_model.ZModel(MMt, ind)
        if hasattr(backend, "prepare_z"):
            backend.prepare_z(geno, k["zm"], availmemGb)
        return MMt

    return prepare, lambda X: {"zmodel": k["zm"]}, lambda m: np.ravel(m)[ind], lambda: {"invMMt": None, "Zmat": k["zm"]}


def _z_rows(trait, currentX, geno, Zmat, backend, say):
    """The checks and the NA handling of AM(Zmat=) -> trait, X, ind_of_obs, geno, indxNA, indxNA_obs.

    Checks as check_inputs_mlam.R:122-145.  A record with NaN in trait or X is dropped (from trait, X and Z; the result's
    indxNA_obs, 1-based, largest first); an individual left without any record is dropped from the genotypes through
    backend.reshape (indxNA, as in AM(); the reference's complete == FALSE rule) and the others are renumbered."""
    n_ind = int(geno["dim_of_ascii_M"][0])
    Zm = np.asarray(Zmat)
    if Zm.ndim == 2 and Zm.shape[1] != n_ind:                                        # check_inputs_mlam.R:124-130
        raise ValueError("Error: the number of columns specified in the Z matrix file is %d\n"
                         "       the number of rows specified in the genotype file is %d\n"
                         "       The number of columns in the Z matrix should be the same as the number of rows in the genotype file."
                         % (Zm.shape[1], n_ind))
    if Zm.shape[0] != trait.size:                                                    # check_inputs_mlam.R:139-145
        raise ValueError("Error: the number of rows specified in the Z matrix file is %d\n"
                         "       the number of rows specified in the phenotype file is %d\n"
                         "       The number of rows in the Z matrix file and phenotype file must be the same." % (Zm.shape[0], trait.size))
    if currentX.shape[0] != trait.size:
        raise ValueError("AM: %d rows of X for %d trait records" % (currentX.shape[0], trait.size))
    ind = as_ind_of_obs(Zm)
    if ind.min() < 0 or ind.max() >= n_ind:
        raise ValueError("AM: Zmat names individual %d, the genotypes hold %d" % (int(ind.max()) + 1, n_ind))
    currentX = currentX.reshape(trait.size, -1)
    trait[np.isnan(currentX).any(axis=1)] = np.nan                                   # AM.R:320-329, per record
    from . import r_api
    indxNA_obs = r_api.check_for_NA_in_trait(trait)
    (trait, currentX, ind), _ = _drop_na_rows(indxNA_obs, (trait, currentX, ind), say=say)
    has = np.bincount(ind, minlength=n_ind) > 0
    indxNA = (np.flatnonzero(~has) + 1)[::-1].copy()                                 # individuals, 1-based, largest first
    if indxNA.size:
        ind = (np.cumsum(has) - 1)[ind]
        say(" The following individuals have no record and are being removed from the genotypes: %s" % " ".join(str(int(i)) for i in indxNA))
        geno = _reshape(geno, indxNA, backend)
    return trait, currentX, ind, geno, indxNA, indxNA_obs


def AM(trait, X, geno, availmemGb=8, ncpu=1, maxit=20, quiet=True, backend=None, message=None, algebra=None, Zmat=None, gamma=1.0):
    """E/R/AM.R:320-475 for a trait vector and a ready design matrix X (n x q, intercept included).

    Individuals whose trait or any column of X is NaN are dropped (AM.R:320-329: an NA covariate makes the trait NA): from trait
    and X, and from the genotype files through backend.reshape(geno, indxNA) (AM.R:345-366; reshape_geno writing the files when
    the backend has no `reshape`).  A trait without NaN makes no such call.
    Returns dict(selected_loci = 1-based marker columns in order of selection, extBIC = list, ve, vg of the last fit, indxNA = the
    dropped rows, 1-based and largest first, and dim_of_ascii_M of the genotypes the loop ran on).
    selected_loci starts as [NA] exactly like AM.R:260, so the selected_loci masking never fires.

    Zmat: repeated measures (several records per genotyped individual), y = X b + Z g + e, as r_api.ReadZmat's matrix or as
    ind_of_obs (r_api.zmat_index); trait and X then have one row per RECORD and Zmat says whose record each is (DESIGN.md section
    4.7c; checks and NA handling: _z_rows, the result also has indxNA_obs).  Variance components and extBIC are emma_REMLE /
    emma_MLE with Z, n = the number of records; the scan runs over the t individuals with operands from Z^T P Z and Z^T P y
    (host_model.scan_operands_z), and a selected marker enters X as Z m_j.  The reference's own AM() cannot run this model (its
    .find_qtl takes no Z): the scan is this project's definition.

    gamma: the weight on extBIC's model-space term (calc_extBIC); 1 is the reference's rule, a smaller value selects more loci.
    FPR4AM finds the gamma of a wanted false positive rate."""
    backend = backend or HipBackend()
    if algebra is not None:  # "host" (LAPACK, the reference's placement) or "device" (rocSOLVER / the fp64 MFMA GEMM through the C ABI)
        host_model.set_algebra(algebra)
    say = message or (lambda *_: None)
    trait = np.asarray(trait, dtype=np.float64).ravel().copy()
    currentX = np.asarray(X, dtype=np.float64)
    extra = {}
    if Zmat is None:
        trait[np.isnan(currentX).reshape(currentX.shape[0], -1).any(axis=1)] = np.nan   # AM.R:320-329
        from . import r_api
        indxNA = r_api.check_for_NA_in_trait(trait)                                     # AM.R:332
        (trait, currentX), geno = _drop_na_rows(indxNA, (trait, currentX), geno, say, backend)
        prepare, fit_kw, column, scan_kw = _plain_model(backend)
    else:
        trait, currentX, ind, geno, indxNA, extra["indxNA_obs"] = _z_rows(trait, currentX, geno, Zmat, backend, say)
        prepare, fit_kw, column, scan_kw = _z_model(backend, ind)
    nmarkers = geno["dim_of_ascii_M"][1]
    s = _loop_state()
    MMt = None
    while s["cont"]:
        say("Iteration %d: Searching for most significant marker-trait association" % s["itnum"])
        new = s["sel"][-1]
        if not (isinstance(new, float) and math.isnan(new)):  # constructX.R:10-22: NA, no pick yet
            currentX = np.column_stack([currentX, column(backend.extract_geno(geno, int(new)).astype(np.float64))])
        if s["itnum"] == 1:
            MMt = prepare(geno, availmemGb, ncpu, np.array(s["sel"]), quiet)
        kw = fit_kw(currentX)  # shared by REMLE and MLE of this iteration (same K, X)
        s["best"] = calcVC(trait, currentX, MMt, **kw)
        s["ext"].append(calc_extBIC(trait, currentX, MMt, nmarkers, gamma=gamma, **kw))
        if _still_improving(s["ext"]):
            s["sel"].append(backend.find_qtl(geno=geno, availmemGb=availmemGb, selected_loci=np.array(s["sel"]), MMt=MMt,
                                             best_ve=s["best"]["ve"], best_vg=s["best"]["vg"], currentX=currentX, ncpu=ncpu,
                                             quiet=quiet, trait=trait, **scan_kw()))
        else:
            s["cont"] = False
        _end_iteration(s, maxit)
    return dict(_AM_result(s, maxit, indxNA, geno), **extra)


def AM_traits(Y, X, geno, availmemGb=8, maxit=20, quiet=True, message=None, algebra=None, device=0, Zmat=None, gamma=1.0):
    """AM() for the T columns of Y (n x T) with one design matrix X (n x q) on one genotype panel, in one run: calcMMt and
    lam, U = eigh(MM^T) once, Z = Mt U once (spectral_prepare), then the traits in lockstep -- each round one spectral_scan_traits
    call for every trait still running, and per trait emma_REMLE_eig / emma_MLE_eig in the eigenbasis (no n^3 work per trait or
    iteration).  Each trait follows AM()'s loop (stop rule AM.R:448, maxit, result assembly AM.R:476-499) and gets a dict with
    AM()'s keys.

    A row with NaN in ANY trait or in X is dropped for ALL traits (one VIEW reshape of the genotypes): with different NA patterns
    the result differs from separate AM() runs, which drop each trait's own NA rows only.  A pick adds its row of Z (U^T m_j,
    spectral_rows) to that trait's U^T X.

    Zmat (repeated measures) is not supported here: the per-trait EMMA in the eigenbasis and the batched kernel's own C would need
    AM(Zmat=)'s within-individual terms.  Run AM(Zmat=) per trait.

    gamma: the weight on extBIC's model-space term, as in AM()."""
    if Zmat is not None:
        raise NotImplementedError("AM_traits: Zmat (repeated measures) is not supported; run AM(Zmat=) for each trait")
    from . import r_api, rcpp_api
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y.reshape(Y.shape[0], -1).copy()
    currentX = np.asarray(X, dtype=np.float64).reshape(Y.shape[0], -1)
    T, q = Y.shape[1], currentX.shape[1]
    if q + maxit - 1 > 31:
        raise ValueError("AM_traits: q + maxit - 1 = %d fixed-effect columns in the last scan; the spectral scan takes at most 31"
                         % (q + maxit - 1))
    if algebra is not None:
        host_model.set_algebra(algebra)
    say = message or (lambda *_: None)
    na_row = np.isnan(Y).any(axis=1) | np.isnan(currentX).any(axis=1)
    indxNA = r_api.check_for_NA_in_trait(np.where(na_row, np.nan, 0.0))
    (Y, currentX), geno = _drop_na_rows(indxNA, (Y, currentX), geno, say, device=device)
    n, nmarkers = geno["dim_of_ascii_M"]
    MMt = r_api.calcMMt(geno, availmemGb, 1, np.array([np.nan]), quiet, device=device)
    lam, U = host_model.algebra().eigh(MMt)
    lam = np.ascontiguousarray(lam)
    del MMt
    rcpp_api.spectral_prepare(geno["asciifileMt"], (nmarkers, n), U, availmemGb, device=device)
    UtY = U.T @ Y
    UtX0 = U.T @ currentX
    del U
    st = [_loop_state(UtX=UtX0) for _ in range(T)]
    while any(s["cont"] for s in st):
        active = [s for s in st if s["cont"]]
        scan = []
        for t, s in enumerate(st):
            if not s["cont"]:
                continue
            say("Trait %d, iteration %d: Searching for most significant marker-trait association" % (t + 1, s["itnum"]))
            r = emma_REMLE_eig(lam, s["UtX"], UtY[:, t])                                         # calcVC
            s["best"] = {k: r[k] for k in ("vg", "ve")}
            ml = emma_MLE_eig(lam, s["UtX"], UtY[:, t], llim=-100, ulim=100)                     # calc_extBIC
            s["ext"].append(_extBIC(ml["ML"], s["UtX"].shape[1], n, nmarkers, gamma))
            if _still_improving(s["ext"]):
                scan.append(t)
            else:
                s["cont"] = False
        if scan:
            res = rcpp_api.spectral_scan_traits(lam, [st[t]["UtX"] for t in scan], UtY[:, scan], [st[t]["best"]["ve"] for t in scan],
                                                [st[t]["best"]["vg"] for t in scan], nmarkers, device=device)
            if np.any(res["index"] < 1):
                raise RuntimeError("AM_traits: every tsq of a scan is NaN")
            rows = rcpp_api.spectral_rows(res["index"] - 1, device=device)
            for j, t in enumerate(scan):
                st[t]["sel"].append(int(res["index"][j]))
                st[t]["UtX"] = np.column_stack([st[t]["UtX"], rows[:, j]])
        for s in active:
            _end_iteration(s, maxit)
    return [_AM_result(s, maxit, indxNA, geno) for s in st]


# ---------------------------------------------------------------------------------------------------------------------------
# FPR4AM: the gamma of a wanted false positive rate, from permutations of the trait.  Not in the reference
# tree (1.0.3); defined from the model.  For a permuted trait y_r AM() selects a (false) locus iff extBIC[1] < extBIC[0] (AM.R:448),
# which with q = ncol(X) and c = lchoose(L, q) - lchoose(L, q - 1) is gamma < gamma_star_r = (2 (ML1_r - ML0_r) - log n) / (2 c).
# ---------------------------------------------------------------------------------------------------------------------------
def fpr_curve(gamma_star, gammas):
    """FPR(gamma) = #{r : gamma_star_r > gamma} / R for every gamma of gammas: a step function that does not increase."""
    gs = np.asarray(gamma_star, dtype=np.float64).ravel()
    g = np.atleast_1d(np.asarray(gammas, dtype=np.float64))
    return (gs[None, :] > g.reshape(-1, 1)).sum(axis=1).reshape(g.shape) / gs.size


def choose_gamma(gamma_star, falseposrate):
    """The smallest gamma >= 0 with FPR(gamma) <= falseposrate: the k-th largest gamma_star, k = floor(falseposrate R) + 1, clipped
    below at 0.  k - 1 is found as the largest count m with m / R <= falseposrate, the comparison fpr_curve's values meet, so that
    a product falseposrate R that rounds below its integer value does not move k."""
    gs = np.asarray(gamma_star, dtype=np.float64).ravel()
    R = gs.size
    if R < 1 or not 0 < falseposrate < 1:
        raise ValueError("choose_gamma: at least one gamma_star and 0 < falseposrate < 1")
    m = int(math.floor(falseposrate * R))
    while (m + 1) / R <= falseposrate:
        m += 1
    while m / R > falseposrate:
        m -= 1
    return max(float(np.sort(gs)[::-1][m]), 0.0)


def _fpr_group(q):
    """Traits with q fixed-effect columns that one pass over Z scores (eagle_spectral_traits_passes)."""
    from . import rcpp_api
    g = 1
    while g < 128 and rcpp_api.spectral_traits_passes([q] * (g + 1)) == 1:
        g += 1
    return g


def FPR4AM(trait, X, geno, falseposrate=0.05, numreps=200, seed=101, availmemGb=8, quiet=True, message=None, algebra=None, device=0,
           eig=None, chunk=None):
    """The weight gamma on extBIC's model-space term at which AM(trait, X, geno, gamma=...) returns a false positive for the share
    falseposrate of traits without any association, estimated from numreps permutations of the trait.

    Rows with NaN in trait or X are dropped first (AM()'s rule, one VIEW reshape).  Permutation r is y[pi_r] with
    pi_r = rng.permutation(n), rng = numpy.random.default_rng(seed), drawn in order r = 0 .. numreps - 1; X and the genotypes stay.
    For each: the null fit on X (REML -> ve, vg; ML -> ML0), the scan's pick j_r, the ML fit on [X | m_j] (ML1) -- iterations 1 and 2
    of AM(y_r, X, geno, maxit=2) -- and gamma_star_r (above).  One calcMMt and one eigh (none with eig = (lam, U) of K, what
    SpectralBackend().eig holds), one spectral_prepare (none when rcpp_api.spectral_holds this Z), then per chunk of `chunk`
    permutations (default: whole column groups of the batched scan, as many as keep the stacked grid products within availmemGb / 8)
    one U^T Y, the batched EMMA, one spectral_scan_traits and one spectral_rows.  Nothing of size numreps x L exists.

    Returns dict(setgamma = choose_gamma(gamma_star, falseposrate), falseposrate = FPR(setgamma) achieved on these permutations,
    gamma_star, picks (1-based), tsqmax, ML0, ML1, ve, vg: numreps each; indxNA, seed, numreps).  setgamma may exceed 1.
    Permuting y against a structured K is an approximation under population structure (it breaks the trait's own covariance with K)."""
    from . import r_api, rcpp_api
    if not 0 < falseposrate < 1:
        raise ValueError("FPR4AM: falseposrate must lie strictly between 0 and 1, got %r" % (falseposrate,))
    numreps = int(numreps)
    if numreps < 1:
        raise ValueError("FPR4AM: numreps must be at least 1")
    y = np.asarray(trait, dtype=np.float64).ravel().copy()
    X0 = np.asarray(X, dtype=np.float64).reshape(y.size, -1)
    q = X0.shape[1]
    if q > 30:
        raise ValueError("FPR4AM: %d columns of X; at most 30 (the pick makes 31, the most the spectral scan takes)" % q)
    if chunk is not None and int(chunk) < 1:
        raise ValueError("FPR4AM: chunk must be at least 1")
    if algebra is not None:
        host_model.set_algebra(algebra)
    say = message or (lambda *_: None)
    y[np.isnan(X0).any(axis=1)] = np.nan                                             # AM.R:320-329
    indxNA = r_api.check_for_NA_in_trait(y)
    (y, X0), geno = _drop_na_rows(indxNA, (y, X0), geno, say, device=device)
    n, L = (int(v) for v in geno["dim_of_ascii_M"])
    if y.size != n:
        raise ValueError("FPR4AM: %d trait records for %d genotyped individuals" % (y.size, n))
    la = host_model.algebra()
    if eig is None:
        MMt = r_api.calcMMt(geno, availmemGb, 1, np.array([np.nan]), quiet, device=device)
        lam, U = la.eigh(MMt)
        del MMt
    else:
        lam, U = eig
        if np.size(lam) != n or np.shape(U) != (n, n):
            raise ValueError("FPR4AM: eig holds %d eigenvalues, the genotypes %d individuals" % (np.size(lam), n))
    lam = np.ascontiguousarray(lam, dtype=np.float64).ravel()
    if not rcpp_api.spectral_holds(geno["asciifileMt"], U, device=device):
        rcpp_api.spectral_prepare(geno["asciifileMt"], (L, n), U, availmemGb, device=device)
    UtX = la.mm(U.T, X0)
    if chunk is None:
        g = _fpr_group(q)
        pairs = (q + 2) * (q + 3) // 2                                               # column products of [X | m_j | y]
        chunk = max(g, int(availmemGb * 2.0 ** 30 / 8 / (8.0 * n * pairs)) // g * g)
    chunk = int(chunk)
    c = _lchoose(L, q) - _lchoose(L, q - 1)
    rng = np.random.default_rng(seed)
    out = {k: np.zeros(numreps) for k in ("gamma_star", "tsqmax", "ML0", "ML1", "ve", "vg")}
    picks = np.zeros(numreps, dtype=np.int64)
    for r0 in range(0, numreps, chunk):
        r1 = min(r0 + chunk, numreps)
        say("Permutations %d to %d of %d" % (r0 + 1, r1, numreps))
        Yc = np.column_stack([y[rng.permutation(n)] for _ in range(r0, r1)])
        UtY = la.mm(U.T, Yc)
        vc = emma_REMLE_eig_batch(lam, UtX, UtY)                                     # calcVC of iteration 1
        ml0 = emma_MLE_eig_batch(lam, UtX, UtY, llim=-100, ulim=100)                 # calc_extBIC of iteration 1
        res = rcpp_api.spectral_scan_traits(lam, [UtX] * (r1 - r0), UtY, vc["ve"], vc["vg"], L, device=device)
        if np.any(res["index"] < 1):
            raise RuntimeError("FPR4AM: every tsq of a scan is NaN")
        uniq, inv = np.unique(np.asarray(res["index"], dtype=np.int64) - 1, return_inverse=True)
        rows = rcpp_api.spectral_rows(uniq, device=device)                           # U^T m_j of the distinct picks
        ml1 = emma_MLE_eig_batch(lam, UtX, UtY, last=rows[:, inv], llim=-100, ulim=100)   # calc_extBIC of iteration 2
        picks[r0:r1] = res["index"]
        for k, v in (("tsqmax", res["tsqmax"]), ("ML0", ml0["ML"]), ("ML1", ml1["ML"]), ("ve", vc["ve"]), ("vg", vc["vg"])):
            out[k][r0:r1] = v
    out["gamma_star"] = (2.0 * (out["ML1"] - out["ML0"]) - math.log(n)) / (2.0 * c)
    setgamma = choose_gamma(out["gamma_star"], falseposrate)
    out.update({"setgamma": setgamma, "falseposrate": float(fpr_curve(out["gamma_star"], setgamma)[0]), "picks": picks,
                "indxNA": indxNA, "seed": seed, "numreps": numreps})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# SummaryAM (E/R/summary_am.R:78-221) in the eigenbasis of K.  Every model of summary_am.R uses K = MMt/max(MMt) + 0.95 I
# (.calcMMt, :140) or K'' = K/max(K) + 0.05 I (:186): with K = U diag(lam) U^T both share U, K'' having lam'' = lam/max(K) + 0.05.
# So with F = [X | m_j1 .. m_jk] (constructX, :131-137), Ft = U^T F and ut = U^T y:
#     H^-1 = U diag(D) U^T, D = 1/(vg lam + ve)   ->   F^T H^-1 F = Ft^T D Ft = A,   F^T H^-1 y = Ft^T D ut     (:149-151)
#     W_j = beta_j^2 / (A^-1)_jj                                                                                   (:155-159)
# and emma.REMLE (:143) / the k + 1 emma.MLE fits (:188, :205) are emma_REMLE_eig / emma_MLE_eig on leading column blocks of Ft.
# One eigh of K (none when the caller holds lam, U) instead of solve(H) and 2k + 3 n x n eigen() calls.
# ---------------------------------------------------------------------------------------------------------------------------
_SUMMARY_NONE = (" No significant marker-trait associations have been found by AM. \n", " Nothing to summarize. \n")   # :117-121


def _summary_names(q, xnames, map, L):
    """colnames of baseX (xnames; default "intercept", "X2", ...) and a function j (1-based) -> marker name: map's names (a
    sequence of L names, or a mapping with an "SNP" entry), by default M1 .. ML as summary_am.R:106-114."""
    xn = ["intercept"] + ["X%d" % j for j in range(2, q + 1)] if xnames is None else [str(v) for v in xnames]
    if len(xn) != q:
        raise ValueError("SummaryAM: %d xnames for %d columns of X" % (len(xn), q))
    if map is None:
        return xn, lambda j: "M%d" % j
    snp = list(map["SNP"]) if hasattr(map, "keys") else list(map)
    if len(snp) != L:
        raise ValueError("SummaryAM: map names %d markers, the genotypes hold %d" % (len(snp), L))
    return xn, lambda j: str(snp[j - 1])


def _summary_eig(lam, maxK, Ft, ut, q, names, say):
    """summary_am.R:142-217 from lam (eigenvalues of K), max(K), Ft = U^T [X | m_j1 .. m_jk] (n x (q + k)) and ut = U^T y."""
    lam = np.ascontiguousarray(lam, dtype=np.float64).ravel()
    n, p = Ft.shape
    eR = emma_REMLE_eig(lam, Ft, ut, llim=-100, ulim=100)                                         # :143
    D = 1.0 / (eR["vg"] * lam + eR["ve"])                                                          # :149-150
    FD = Ft * D[:, None]
    Ainv = np.linalg.inv(Ft.T @ FD)
    beta = Ainv @ (FD.T @ ut)                                                                      # :151
    W = beta * beta / np.diag(Ainv)                                                                # :157-159
    pval = 1.0 - chdtr(1, W)                                                                       # :160, 1 - pchisq(W, 1)
    say(" ~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~ \n")
    say("     Size and Significance of Effects in Final Model    \n")
    say(" ~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~ \n")
    say("%15s  %10s  %10s \n" % ("Name", "Additive effect", "p-value"))
    for nm, b, pv in zip(names, beta, pval):
        say("%15s  %10f         %.3E\n" % (nm, b, pv))
    say("\n\n\n")
    lam2 = lam / maxK + 0.05                                                                       # :186
    base = emma_MLE_eig(lam2, Ft[:, :q], ut, llim=-100, ulim=100)["ML"]                            # :188
    say(" ~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~ \n")
    say(" Proportion of Phenotype Variance Explained by Multiple-locus \n")
    say("             Association Mapping Model \n")
    say("  Marker loci which were found by AM() are added one at a time    \n")
    say(" ~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~ \n")
    say("   %15s      %10s \n" % ("Marker name", "Proportion"))
    rnames, rsq = [], []
    for k in range(q + 1, p + 1):                                                                  # :200-211
        full = emma_MLE_eig(lam2, Ft[:, :k], ut, llim=-100, ulim=100)["ML"]
        rsq.append(1.0 - math.exp(-2.0 / n * (full - base)))
        say("  %+15s          %.3f\n" % ("+  " + names[k - 1], rsq[-1]))
        rnames.append("+ " + names[k - 1])
    pval = [float(v) for v in pval]
    return {"pvalue": {"effects": list(names), "p_value": pval, "W": [float(v) for v in W]},
            "size": {"effect_names": list(names), "estimate": [float(v) for v in beta], "p_value": list(pval)},
            "R": {"Marker_name": rnames, "Prop_var_explained": rsq}}


def _say_none(say):
    """The two messages of a model without picks -> None, what its summary is."""
    for m in _SUMMARY_NONE:
        say(m)


def _summary_setup(who, indxNA, arrays, geno, map, xnames, availmemGb, eig, backend):
    """What SummaryAM and SummaryAM_traits share once a trait has a pick: the rows indxNA leave `arrays` (X first) and the genotypes
    (backend.reshape, or reshape_geno writing files for a backend without one); the names; K by calcMMt with selected_loci = NA
    (summary_am.R:140; the masking never fires), max(K), and lam, U: eig when given, else one eigh of K.
    -> arrays, geno, colnames of X, j -> marker name, max(K), lam, U."""
    arrays, geno = _drop_na_rows(indxNA, arrays, geno, backend=backend)
    n, L = geno["dim_of_ascii_M"]
    if arrays[0].shape[0] != n:
        raise ValueError("%s: %d trait records for %d genotyped individuals" % (who, arrays[0].shape[0], n))
    xn, mname = _summary_names(arrays[0].shape[1], xnames, map, L)
    K = backend.calcMMt(geno, availmemGb, 1, np.array([np.nan]), True)
    maxK = float(np.max(K))
    if eig is None:
        lam, U = host_model.algebra().eigh(K)
    else:
        lam, U = eig
        if np.size(lam) != n or np.shape(U) != (n, n):
            raise ValueError("SummaryAM: eig holds %d eigenvalues, the genotypes %d individuals" % (np.size(lam), n))
    return arrays, geno, xn, mname, maxK, np.ascontiguousarray(lam, dtype=np.float64).ravel(), U


def tag_markers(AMobj, geno, r2=0.8, map=None, availmemGb=8, device=0):
    """Which markers tag each locus AM() picked -> one dict per entry of AMobj["selected_loci"], in that order:
    {"locus": the pick, "markers": the markers with r^2 >= r2 to it, the pick included (both 1-based, as AM() reports loci; int64,
    increasing), "r2": their r^2}, and with a map (ReadBim's dict; names alone give only "names") "names", "chrom" (the pick's) and
    "span" = (lowest, highest position of the tagging markers on that chromosome).  geno is what AM() was given: the individuals
    AMobj["indxNA"] are left out as AM() left them out (a view on `device`).  The dot products run on the device (r_api.LDofLoci)."""
    from . import r_api
    picks = [int(j) for j in AMobj["selected_loci"]]
    if not picks:
        return []
    indxNA = np.asarray(AMobj.get("indxNA", ()), dtype=np.int64).ravel()
    if indxNA.size:
        geno = _reshape(geno, indxNA, None, device)
    ld = r_api.LDofLoci(geno, [j - 1 for j in picks], availmemGb=availmemGb, device=device)
    L = ld["r2"].shape[0]
    names = chrom = pos = None
    if map is not None:
        names = list(map["SNP"]) if hasattr(map, "keys") else list(map)
        if len(names) != L:
            raise ValueError("tag_markers: map names %d markers, the genotypes hold %d" % (len(names), L))
        if hasattr(map, "keys") and "Chr" in map and "Pos" in map:
            chrom, pos = np.asarray(map["Chr"]), np.asarray(map["Pos"])
    out = []
    for c, j in enumerate(picks):
        col = ld["r2"][:, c]
        hit = np.nan_to_num(col, nan=-1.0) >= float(r2)
        hit[j - 1] = True
        idx = np.flatnonzero(hit)
        e = {"locus": j, "markers": idx.astype(np.int64) + 1, "r2": col[idx]}
        if names is not None:
            e["names"] = [str(names[i]) for i in idx]
        if chrom is not None:
            same = idx[chrom[idx] == chrom[j - 1]]
            e["chrom"] = chrom[j - 1].item() if hasattr(chrom[j - 1], "item") else chrom[j - 1]
            e["span"] = (pos[same].min().item(), pos[same].max().item())
        out.append(e)
    return out


def SummaryAM(AMobj, trait, X, geno, map=None, xnames=None, availmemGb=8, eig=None, backend=None, message=None, device=0):
    """summary_am.R:78-221 for the dict AM() returns; r_api.SummaryAM, which forwards here, documents arguments and result.  The
    rows to drop are AMobj["indxNA"]; the marker columns come from extract_geno and enter one product U^T [X | m_j1 .. m_jk | y]."""
    say = message or (lambda *_: None)
    picks = [int(j) for j in AMobj["selected_loci"]]
    if not picks:
        return _say_none(say)
    backend = backend or HipBackend(device)
    y = np.asarray(trait, dtype=np.float64).ravel()
    X = np.asarray(X, dtype=np.float64).reshape(y.size, -1)
    indxNA = np.asarray(AMobj.get("indxNA", ()), dtype=np.int64).ravel()
    (X, y), geno, xn, mname, maxK, lam, U = _summary_setup("SummaryAM", indxNA, (X, y), geno, map, xnames, availmemGb, eig, backend)
    q = X.shape[1]
    F = np.column_stack([X] + [backend.extract_geno(geno, j).astype(np.float64) for j in picks] + [y])   # constructX, :131-137
    Ft = host_model.algebra().mm(U.T, F)
    return _summary_eig(lam, maxK, Ft[:, :-1], Ft[:, -1], q, xn + [mname(j) for j in picks], say)


def SummaryAM_traits(results, Y, X, geno, map=None, xnames=None, availmemGb=8, eig=None, backend=None, message=None, device=0):
    """r_api.SummaryAM for every entry of AM_traits(Y, X, geno)'s result, with one calcMMt and one eigh (none with eig=) for
    all traits.  The rows are AM_traits': a row with NaN in any trait or in X is dropped for all traits (backend.reshape, or
    reshape_geno writing files for a backend without one).  The marker columns of U^T F come from the resident Z (spectral_rows)
    when it was made from these genotypes with exactly this U -- the AM_traits run's context still open --, else from one
    host_model.algebra().mm over the union of all traits' picks.  Returns a list of SummaryAM results (None for a trait with no
    pick)."""
    from . import r_api, rcpp_api
    say = message or (lambda *_: None)
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y.reshape(Y.shape[0], -1)
    X = np.asarray(X, dtype=np.float64).reshape(Y.shape[0], -1)
    if len(results) != Y.shape[1]:
        raise ValueError("SummaryAM_traits: %d results for %d traits" % (len(results), Y.shape[1]))
    picks = [[int(j) for j in r["selected_loci"]] for r in results]
    if not any(picks):
        return [_say_none(say) for _ in picks]
    backend = backend or HipBackend(device)
    na_row = np.isnan(Y).any(axis=1) | np.isnan(X).any(axis=1)
    indxNA = r_api.check_for_NA_in_trait(np.where(na_row, np.nan, 0.0))
    (X, Y), geno, xn, mname, maxK, lam, U = _summary_setup("SummaryAM_traits", indxNA, (X, Y), geno, map, xnames, availmemGb, eig, backend)
    q = X.shape[1]
    la = host_model.algebra()
    UtXY = la.mm(U.T, np.column_stack([X, Y]))
    union = sorted({j for pk in picks for j in pk})
    if rcpp_api.spectral_holds(geno["asciifileMt"], U, device=device):
        UtM = rcpp_api.spectral_rows(np.asarray(union) - 1, device=device)
    else:
        UtM = la.mm(U.T, np.column_stack([backend.extract_geno(geno, j).astype(np.float64) for j in union]))
    col = {j: i for i, j in enumerate(union)}
    out = []
    for t, pk in enumerate(picks):
        if not pk:
            out.append(_say_none(say))
            continue
        Ft = np.column_stack([UtXY[:, :q], UtM[:, [col[j] for j in pk]]])
        out.append(_summary_eig(lam, maxK, Ft, UtXY[:, q + t], q, xn + [mname(j) for j in pk], say))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# GWAS: the single-locus mixed-model scan (no counterpart in the reference, whose AM() reports the loci of ONE multi-locus model): a
# row per marker for the Manhattan plot and the comparison the Eagle paper draws between AM()'s picks and a single-locus scan.  Two
# tests of gamma = 0 in y = X beta + m_i gamma + g + e on the Z that SpectralBackend keeps resident: the score test under the null
# model's variance components (EMMAX / P3D; one eagle_spectral_scan) and the exact test with delta re-estimated per marker (GEMMA /
# FaST-LMM; eagle_spectral_lmm, include/eagle_hip.h section 1d').
# ---------------------------------------------------------------------------------------------------------------------------
_GWAS_EXACT = ("beta", "se", "stat", "p", "delta", "vg", "ve", "ll")


def _null_model(who, trait, X, geno, backend, availmemGb, device, map=None, ml=False, min_df=2):
    """What GWAS and SetTest share: the records without NaN in trait or X (a VIEW reshape, as AM() drops them), the backend's K = U
    diag(lam) U^T and resident Z = Mt U -- reused when the backend already holds them for these genotypes, built otherwise --, Ut =
    U^T X, ut = U^T y and the null fit on X alone (emma_REMLE_eig; with ml=True emma_MLE_eig as well) -> dict(backend, geno, y, X, n, L,
    c, lam, U, Ut, ut, null = {"reml", "ml"}, indxNA, names).  n > c + min_df is required."""
    from . import r_api, rcpp_api
    backend = backend or SpectralBackend(device)
    if not hasattr(backend, "eig"):
        raise TypeError("%s: the backend must be an am.SpectralBackend (it keeps Z = Mt U resident)" % who)
    y = np.asarray(trait, dtype=np.float64).ravel().copy()
    Xa = np.asarray(X, dtype=np.float64).reshape(y.size, -1)
    c = Xa.shape[1]
    if not 1 <= c <= rcpp_api.LMM_MAX_COVARIATES:
        raise ValueError("%s: X must hold 1 to %d columns, the intercept included" % (who, rcpp_api.LMM_MAX_COVARIATES))
    y[np.isnan(Xa).any(axis=1)] = np.nan                                             # AM.R:320-329
    indxNA = r_api.check_for_NA_in_trait(y)
    (y, Xa), geno = _drop_na_rows(indxNA, (y, Xa), geno, backend=backend, device=backend.device)
    n, L = (int(v) for v in geno["dim_of_ascii_M"])
    if y.size != n:
        raise ValueError("%s: %d trait records for %d genotyped individuals" % (who, y.size, n))
    if n <= c + min_df:
        raise ValueError("%s: %d individuals for %d columns of X" % (who, n, c))
    names = None if map is None else _summary_names(c, None, map, L)[1]
    if backend.eig is None or backend.lam.size != n or not rcpp_api.spectral_holds(geno["asciifileMt"], backend.U, device=backend.device):
        backend.calcMMt(geno, availmemGb, 1, np.array([np.nan]), True)                # K, its eigh and Z = Mt U
    lam, U = backend.eig
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    la = host_model.algebra()
    Ut, ut = la.mm(U.T, Xa), U.T @ y
    fit = {"reml": emma_REMLE_eig(lam, Ut, ut)}
    fit["ml"] = emma_MLE_eig(lam, Ut, ut) if ml else None
    null = {m: None if r is None else {"delta": r["delta"], "vg": r["vg"], "ve": r["ve"], "ll": r["REML" if m == "reml" else "ML"]}
            for m, r in fit.items()}
    if not null["reml"]["vg"] > 0:
        raise ValueError("%s: the null model has no fit (collinear columns of X?)" % who)
    return {"backend": backend, "geno": geno, "y": y, "X": Xa, "n": n, "L": L, "c": c, "lam": lam, "U": U, "Ut": Ut, "ut": ut, "null": null,
            "indxNA": indxNA, "names": names}


def GWAS(trait, X, geno, exact="all", method="reml", p_exact=None, map=None, backend=None, availmemGb=8, device=0, Zmat=None):
    """Per-marker tests of a quantitative trait under the mixed model; r_api.GWAS forwards here.

    trait (n, NaN = no record), X (n x c, 1 <= c <= 14, the intercept column included), geno: as AM() takes them; rows with NaN in
    trait or X are dropped as AM() drops them (a VIEW reshape).  backend: an am.SpectralBackend (default: a new one on `device`).  One
    that already ran on these genotypes -- AM(trait, X, geno, backend=b) -- still holds lam, U and the resident Z: nothing is rebuilt.

    Returns a dict of fp64 (L) columns unless noted:
      "score" = a^2 / vara, "p_score" = chdtrc(1, score), "beta_p3d" = vg a / vara: the P3D test of every marker under the REML
        null fit (emma_REMLE_eig on X alone), from one spectral_scan;
      "beta", "se", "stat", "p", "delta", "vg", "ve", "ll", "code" (int32), "iterations" (int32): the exact test (section 1d' of the
        header) started at the null fit's ln delta, for every marker (exact="all"), for none (exact="none") or, with p_exact, for
        the markers with p_score < p_exact only -- the others keep NaN and code -1.  method="reml": stat = (beta / se)^2, p =
        fdtrc(1, n - c - 1, stat) (Wald); method="ml": stat = 2 (ll - the null ML fit's ll), p = chdtrc(1, stat).  Markers whose code
        is 2 hold NaN.  This is the optimum reached from the null fit, not emma's search over a grid;
      "null": {"delta", "vg", "ve", "ll"} of the method's null fit (emma_REMLE_eig / emma_MLE_eig), "null_reml": the same of the REML
        fit the P3D columns use, "lambda_gc" = median(score) / 0.4549... (the chi^2_1 median), "n_used", "indxNA" and, with map= (L
        names or a mapping with "SNP"), "names".
    Zmat (repeated measures) is not supported."""
    from scipy.special import chdtrc, chdtri, fdtrc
    from . import r_api, rcpp_api
    if Zmat is not None:
        raise NotImplementedError("GWAS: Zmat (repeated measures) is not supported: the exact test has no within-individual terms")
    if exact not in ("all", "none") or method not in ("reml", "ml"):
        raise ValueError("GWAS: exact must be \"all\" or \"none\", method \"reml\" or \"ml\"")
    if p_exact is not None and not 0.0 < float(p_exact) <= 1.0:
        raise ValueError("GWAS: p_exact must lie in (0, 1]")
    nm = _null_model("GWAS", trait, X, geno, backend, availmemGb, device, map=map, ml=method == "ml")
    backend, n, L, c, lam, Ut, ut, null, indxNA, names = (nm[k] for k in ("backend", "n", "L", "c", "lam", "Ut", "ut", "null", "indxNA", "names"))
    res = rcpp_api.spectral_scan(lam, Ut, ut, null["reml"]["ve"], null["reml"]["vg"], L, device=backend.device)
    a, vara = res["a"].ravel(), res["vara"].ravel()
    with np.errstate(all="ignore"):
        score = a * a / vara
        out = {"score": score, "p_score": chdtrc(1.0, score), "beta_p3d": null["reml"]["vg"] * a / vara}
    for k in _GWAS_EXACT:
        out[k] = np.full(L, np.nan)
    out["code"], out["iterations"] = np.full(L, -1, dtype=np.int32), np.zeros(L, dtype=np.int32)
    idx = None if p_exact is None else np.flatnonzero(out["p_score"] < float(p_exact))
    if exact == "all" and (idx is None or idx.size):
        stat, info = rcpp_api.spectral_lmm(lam, Ut, ut, reml=method == "reml", theta0=math.log(null[method]["delta"]), idx=idx,
                                           n_markers=L, device=backend.device)
        rows = slice(None) if idx is None else idx
        for j, k in enumerate(("beta", "se", "delta", "vg", "ll")):
            out[k][rows] = stat[:, j]
        out["code"][rows], out["iterations"][rows] = info[:, 0], info[:, 1]
        out["ve"] = out["delta"] * out["vg"]
        with np.errstate(all="ignore"):
            if method == "reml":
                out["stat"] = (out["beta"] / out["se"]) ** 2
                out["p"] = fdtrc(1.0, float(n - c - 1), out["stat"])
            else:
                out["stat"] = np.where(np.isnan(out["ll"]), np.nan, np.maximum(2.0 * (out["ll"] - null["ml"]["ll"]), 0.0))
                out["p"] = chdtrc(1.0, out["stat"])
    out.update({"null": null[method], "null_reml": null["reml"], "lambda_gc": float(np.nanmedian(score) / chdtri(1.0, 0.5)), "n_used": n,
                "indxNA": indxNA, "method": method})
    if names is not None:
        out["names"] = [names(j) for j in range(1, L + 1)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# SetTest: is a gene, a window or a candidate region AS A WHOLE associated with the trait?  The burden test and SKAT under the null
# model GWAS uses (the EMMAX-SKAT / famSKAT tests; no counterpart in the reference): the scores of a set's markers and their
# covariance varG^2 m_i' P m_j from one eagle_spectral_settest over the resident Z (include/eagle_hip.h section 1d''), the p-values
# on the host.
# ---------------------------------------------------------------------------------------------------------------------------
def _set_weights(weights, L, geno, availmemGb, device):
    """One weight per marker of the panel: "equal", ("beta", a, b) / "beta" (Beta(MAF; a, b), default (1, 25)) or an array of L."""
    from . import r_api
    if isinstance(weights, str) and weights == "equal":
        return np.ones(L)
    if (isinstance(weights, str) and weights == "beta") or (isinstance(weights, tuple) and len(weights) in (1, 3) and weights[0] == "beta"):
        from scipy.stats import beta
        a, b = (1.0, 25.0) if isinstance(weights, str) or len(weights) == 1 else (float(weights[1]), float(weights[2]))
        if not (a > 0.0 and b > 0.0):
            raise ValueError("SetTest: the Beta weights need a, b > 0")
        maf = np.asarray(r_api.MarkerStats(geno, availmemGb=availmemGb, device=device)["maf"], dtype=np.float64)
        w = beta.pdf(np.nan_to_num(maf, nan=0.0), a, b)
        return np.where(np.isfinite(w) & ~np.isnan(maf), w, 0.0)
    if isinstance(weights, (str, tuple)):
        raise ValueError("SetTest: weights must be \"equal\", (\"beta\", a, b) or one weight per marker")
    w = np.asarray(weights, dtype=np.float64).ravel()
    if w.size != L or not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
        raise ValueError("SetTest: %d weights, finite and >= 0, for %d markers" % (w.size, L))
    return w


def SetTest(trait, X, geno, sets, weights="equal", p_refine=1e-3, backend=None, map=None, availmemGb=8, device=0, Zmat=None):
    """Burden and SKAT tests of marker sets under the mixed model; r_api.SetTest forwards here.

    trait, X, geno, backend: as GWAS takes them (rows with NaN dropped; a SpectralBackend that AM() or GWAS() already ran on these
    genotypes is reused, nothing is rebuilt).  sets: a list of arrays of 0-based markers, 1 to 64 each, or the dict
    r_api.sets_from_windows / sets_from_table return (its "names" name the sets); a marker may be in many sets.  weights: "equal",
    ("beta", a, b) -- Beta(MAF; a, b) of r_api.MarkerStats, "beta" = (1, 25) -- or one weight per marker of the panel.

    Returns a dict, per set (k entries): "n_markers", "n_used" (markers not degenerate: not monomorphic, not in the span of X),
    "burden" = Ub^2 / Vb, "p_burden" = chdtrc(1, burden), "beta_burden" = vg Ub / Vb (the beta_p3d convention of GWAS), "Q",
    "p_skat_liu" (modified Liu moment matching on the four traces the device returns), "p_skat" (= p_skat_liu, or for the sets with
    p_skat_liu < p_refine the saddlepoint p-value from the eigenvalues of W Phi W, a second device call with cov_out for those sets
    alone), "refined" (bool), "code" (0 ok, 2 nothing left: NaN); and "null" (delta, vg, ve, ll of the REML fit), "names", "n_used_individuals", "indxNA".
    With map= (L names or a mapping with "SNP") also "markers": the marker names of every set.  Zmat (repeated measures) is not supported."""
    from scipy.special import chdtrc
    from . import r_api, rcpp_api
    if Zmat is not None:
        raise NotImplementedError("SetTest: Zmat (repeated measures) is not supported: the set statistics have no within-individual terms")
    if p_refine is not None and not 0.0 <= float(p_refine) <= 1.0:
        raise ValueError("SetTest: p_refine must lie in [0, 1]")
    set_names = list(sets["names"]) if hasattr(sets, "keys") else None
    idx = [np.ascontiguousarray(np.atleast_1d(s), dtype=np.int64) for s in (sets["sets"] if hasattr(sets, "keys") else sets)]
    k = len(idx)
    if set_names is None:
        set_names = ["set%d" % (o + 1) for o in range(k)]
    if len(set_names) != k:
        raise ValueError("SetTest: %d names for %d sets" % (len(set_names), k))
    big = [set_names[o] for o in range(k) if not 1 <= idx[o].size <= rcpp_api.SETTEST_MAX_MARKERS]
    if big:
        raise ValueError("SetTest: every set must hold 1 to %d markers: %s" % (rcpp_api.SETTEST_MAX_MARKERS, ", ".join(big)))
    nm = _null_model("SetTest", trait, X, geno, backend, availmemGb, device, map=map, min_df=1)
    backend, L, lam, Ut, ut, null = nm["backend"], nm["L"], nm["lam"], nm["Ut"], nm["ut"], nm["null"]["reml"]
    if any(s.size and (s.min() < 0 or s.max() >= L) for s in idx):
        raise ValueError("SetTest: the sets hold 0-based markers below %d" % L)
    w = _set_weights(weights, L, nm["geno"], availmemGb, backend.device)
    omega = [w[s] for s in idx]
    res = rcpp_api.spectral_settest(lam, Ut, ut, null["ve"], null["vg"], idx, omega, device=backend.device)
    stat, info = res["stat"], res["info"]
    Q, Ub, Vb = stat[:, 0], stat[:, 1], stat[:, 2]
    with np.errstate(all="ignore"):
        burden = Ub * Ub / Vb
        out = {"n_markers": np.array([s.size for s in idx], dtype=np.int64), "n_used": info[:, 1].astype(np.int64), "burden": burden,
               "p_burden": chdtrc(1.0, burden), "beta_burden": null["vg"] * Ub / Vb, "Q": Q.copy(), "code": info[:, 0].copy()}
    liu = np.array([r_api.skat_pvalue(Q[o], c=stat[o, 3:7]) if info[o, 0] == 0 else np.nan for o in range(k)])
    out["p_skat_liu"], out["p_skat"], out["refined"] = liu, liu.copy(), np.zeros(k, dtype=bool)
    hit = np.flatnonzero(liu < float(p_refine)) if p_refine is not None else np.zeros(0, dtype=np.int64)
    if hit.size:
        cov = rcpp_api.spectral_settest(lam, Ut, ut, null["ve"], null["vg"], [idx[o] for o in hit], [omega[o] for o in hit], cov=True,
                                        device=backend.device)["cov"]
        for o, Phi in zip(hit, cov):
            p = r_api.skat_pvalue(Q[o], eig=np.linalg.eigvalsh(Phi * np.outer(omega[o], omega[o])), method="saddle")
            if p == p:
                out["p_skat"][o], out["refined"][o] = p, True
    out.update({"null": null, "names": set_names, "n_used_individuals": nm["n"], "indxNA": nm["indxNA"]})
    if nm["names"] is not None:
        out["markers"] = [[nm["names"](int(j) + 1) for j in s] for s in idx]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Using the fitted model (no counterpart in the reference, which stops at the loci): BLUPs of the marker effects from one exact
# M^T (P y) on the device (include/eagle_hip.h section 1b''''i) and predictions for any panel with the same markers.
# ---------------------------------------------------------------------------------------------------------------------------
def blup_operands(y, X, K, ve, vg):
    """The mixed-model solutions of y = X b + g + e, g ~ N(0, vg K), e ~ N(0, ve I) -> {"beta", "Py", "ghat"}, host algebra only.
    H = ve I + vg K (host_model.calculateH);  P = H^-1 - H^-1 X (X^T H^-1 X)^-1 X^T H^-1 (host_model.calculateP);
    beta = (X^T H^-1 X)^-1 X^T H^-1 y;  ghat = vg K P y.  They satisfy y - X beta = vg K P y + ve P y  (H P y = y - X beta)."""
    y = np.asarray(y, dtype=np.float64).ravel()
    X = np.asarray(X, dtype=np.float64).reshape(y.size, -1)
    K = np.asarray(K, dtype=np.float64)
    H = host_model.calculateH(K, ve, vg)
    Py = host_model.calculateP(H, X) @ y
    HiX = np.linalg.solve(H, X)
    beta = np.linalg.solve(X.T @ HiX, HiX.T @ y)
    return {"beta": beta, "Py": Py, "ghat": vg * (K @ Py)}


def MarkerEffects(AMobj, trait, X, geno, availmemGb=8, backend=None, device=0):
    """The model AM() selected, refitted and turned into per-marker effects -> {"beta": the fixed effects of [X | the reported loci],
    "loci": AMobj["selected_loci"] (1-based), "u": fp64 (L), the BLUPs of the polygenic marker effects, "weights": u with each locus'
    fixed effect added at its marker (what Predict scores for "genetic"), "ve", "vg", "c", "Py", "ghat", "bound", "nX": the columns of X}.

    trait, X and geno are what AM() was given, NaN included: the rows AMobj["indxNA"] leave trait and X and, as a VIEW, the genotypes
    (SummaryAM's rule).  X gets the reported loci as columns (extract_geno) and the variance components are REFITTED on that model
    (calcVC): after an extBIC stop AMobj["ve"] / ["vg"] belong to the model that still held the dropped last pick.
    AM()'s K is MM^T / max(MM^T) + 0.95 I (calcMMt).  With c = 1 / max(MM^T) and P y of blup_operands,
        ghat = vg K P y = M u + 0.95 vg P y,        u = vg c M^T (P y):
    u is one rcpp_api.marker_scores call of the quantised P y (r_api.quantise_weights, scale s) on the VIEW's Mt file, so every u_m
    errs by at most "bound" = vg c 0.5 n / s.  The 0.95 vg P y term is the part of a TRAINING individual's genetic value that the
    ridge on K's diagonal assigns to that individual alone; it is no function of the genotypes and not part of a prediction."""
    from . import r_api, rcpp_api
    backend = backend or HipBackend(device)
    y = np.asarray(trait, dtype=np.float64).ravel()
    X = np.asarray(X, dtype=np.float64).reshape(y.size, -1)
    indxNA = np.asarray(AMobj.get("indxNA", ()), dtype=np.int64).ravel()
    (X, y), geno = _drop_na_rows(indxNA, (X, y), geno, backend=backend, device=device)
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    if y.size != n:
        raise ValueError("MarkerEffects: %d trait records for %d genotyped individuals" % (y.size, n))
    loci = [int(j) for j in AMobj["selected_loci"]]
    q = X.shape[1]
    Xl = np.column_stack([X] + [backend.extract_geno(geno, j).astype(np.float64) for j in loci])
    K = backend.calcMMt(geno, availmemGb, 1, np.array([np.nan]), True)
    _, mx = rcpp_api.last_mmt_normalised(n, device=device)      # max(MM^T) of the product calcMMt just made
    c = 1.0 / float(mx)
    vc = calcVC(y, Xl, K, eig_R=emma_eigen_R_wo_Z(K, Xl))
    ve, vg = float(vc["ve"]), float(vc["vg"])
    op = blup_operands(y, Xl, K, ve, vg)
    pq, s = r_api.quantise_weights(op["Py"])
    S = rcpp_api.marker_scores(geno["asciifileMt"], (n, L), pq, availmemGb, device=device)[:, 0]
    u = (vg * c) * (S.astype(np.float64) / s)
    w = u.copy()
    for i, j in enumerate(loci):
        w[j - 1] += op["beta"][q + i]
    return {"beta": op["beta"], "loci": loci, "u": u, "weights": w, "ve": ve, "vg": vg, "c": c, "Py": op["Py"], "ghat": op["ghat"],
            "bound": vg * c * 0.5 * float(n) / s, "nX": q}


def Predict(effects, geno, X=None, availmemGb=8, device=0):
    """Genetic values from MarkerEffects' result for the individuals of ANY panel with the same markers in the same order -- the full
    file AM() was given, whose NaN-trait individuals are the selection candidates, or new genotypes -> {"polygenic": M u, "genetic":
    M weights (the polygenic value plus the reported loci's fixed effects)} and, with X (the candidates' rows of the design matrix AM()
    was given, the loci not included), "yhat": X beta_X + genetic.  Two columns of one r_api.Score call.
    For a training individual the model's ghat is polygenic + 0.95 vg P y: that second term belongs to the individual's own record
    (MarkerEffects' docstring) and is not part of a prediction."""
    from . import r_api
    u = np.asarray(effects["u"], dtype=np.float64).ravel()
    L = int(geno["dim_of_ascii_M"][1])
    if u.size != L:
        raise ValueError("Predict: the effects hold %d markers, the panel %d" % (u.size, L))
    sc = r_api.Score(geno, np.column_stack([u, np.asarray(effects["weights"], dtype=np.float64).ravel()]), availmemGb=availmemGb,
                     device=device)
    out = {"polygenic": sc["score"][:, 0], "genetic": sc["score"][:, 1], "bound": sc["bound"]}
    if X is not None:
        X = np.asarray(X, dtype=np.float64).reshape(out["genetic"].size, -1)
        nX = int(effects.get("nX", X.shape[1]))
        if X.shape[1] != nX:
            raise ValueError("Predict: X holds %d columns, the model's design matrix %d" % (X.shape[1], nX))
        out["yhat"] = X @ np.asarray(effects["beta"], dtype=np.float64)[:nX] + out["genetic"]
    return out


def EpistasisOfLoci(AMobj, trait, X, geno, availmemGb=8, backend=None, device=0):
    """Do the loci AM() reported interact with anything in the genome?  r_api.Epistasis(loci = AMobj's loci) on the conditional residual
    P y of the fitted model -> Epistasis' loci-mode dict, with "loci" 0-based, "selected_loci" as AM() reports them (1-based) and "geno":
    the panel of the kept individuals the statistics refer to.

    trait, X and geno are what AM() was given (MarkerEffects' rule for NaN records: they leave as a VIEW).  MarkerEffects refits the
    model with the loci as fixed effects and returns P y; ve P y = y - X beta - ghat is the residual with fixed effects AND the polygenic
    background taken out, so the interaction test is not confounded by relatedness the way a test on the raw trait is.  The F statistic
    does not depend on the scale of its trait, so P y is used as it is (r_api.quantise_trait centres and scales it)."""
    from . import r_api
    backend = backend or HipBackend(device)
    y = np.asarray(trait, dtype=np.float64).ravel()
    X = np.asarray(X, dtype=np.float64).reshape(y.size, -1)
    indxNA = np.asarray(AMobj.get("indxNA", ()), dtype=np.int64).ravel()
    (X, y), kept = _drop_na_rows(indxNA, (X, y), geno, backend=backend, device=device)      # once: MarkerEffects gets the kept records
    eff = MarkerEffects(dict(AMobj, indxNA=()), y, X, kept, availmemGb=availmemGb, backend=backend, device=device)
    loci0 = [int(j) - 1 for j in eff["loci"]]
    if not loci0:
        raise ValueError("EpistasisOfLoci: AM() reported no locus")
    out = r_api.Epistasis(kept, eff["Py"], loci=loci0, availmemGb=availmemGb, device=device)
    out["selected_loci"] = list(eff["loci"])
    out["geno"] = kept
    return out

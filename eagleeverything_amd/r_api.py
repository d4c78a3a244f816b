"""Mirror of the thin R wrappers around the hot calls (argument marshalling is part of parity).

  calculateMMt ........... E/R/calculateMMt.R:3-30
  calcMMt ................ E/R/calcMMt.R:1-15       (.calcMMt)
  calculate_a_and_vara ... E/R/calculate_a_and_vara.R:1-34
  find_qtl ............... E/R/find_qtl.R:1-84      (.find_qtl; host algebra from host_model)
  extract_geno, constructX E/R/extract_geno.R:1-19, E/R/constructX.R:1-24
  ReshapeM ............... E/R/ReshapeM.R:1-11
  check_for_NA_in_trait .. E/R/check_for_NA_in_trait.R:1-25
  ReadZmat ............... E/R/ReadZmat.R:34-111     (zmat_index: the matrix as the vector ind_of_obs)
  SummaryAM .............. E/R/summary_am.R:78-221   (in the eigenbasis of K; am.SummaryAM)
  MarkerStats, FilterMarkers, subset_map ... marker QC, not in the reference (counts on the device, rules on the host)

`geno` is the reference's list {asciifileM, asciifileMt, dim_of_ascii_M = (n, L)} (E/R/ReadMarker.R:306-307).
selected_loci follow R: 1-based, NA = numpy.nan.  The "-1 only if no NA anywhere" rule
(calculateMMt.R:24, calculate_a_and_vara.R:23) is reproduced literally.
"""
import math
import os

import numpy as np

from . import host_model, rcpp_api


def _shift_if_no_na(selected_loci):
    s = np.atleast_1d(np.asarray(selected_loci, dtype=np.float64))
    if not np.any(np.isnan(s)):
        s = s - 1
    return s


def calculateMMt(geno, availmemGb, ncpu, selected_loci=np.nan, dim_of_ascii_M=None, quiet=True, message=None, device=0):
    if not os.path.exists(geno) and not rcpp_api.is_view(geno, device):  # calculateMMt.R:19-23 (a view alias has no file)
        if message:
            message(" Error: The binary packed file %s cannot be found.\n" % geno)
            message(" calculateMMt has terminated with errors.")
        return None
    return rcpp_api.calculateMMt_rcpp(f_name_ascii=geno, selected_loci=_shift_if_no_na(selected_loci),
                                      max_memory_in_Gbytes=availmemGb, num_cores=ncpu, dims=dim_of_ascii_M, quiet=quiet,
                                      message=message, device=device)


def calcMMt(geno, availmemGb, ncpu, selected_loci, quiet, device=0, message=None):
    MMt = calculateMMt(geno=geno["asciifileM"], availmemGb=availmemGb, ncpu=ncpu,
                       dim_of_ascii_M=geno["dim_of_ascii_M"], selected_loci=selected_loci, quiet=quiet, message=message,
                       device=device)
    if MMt is None:
        return None
    # MMt/max(MMt) + diag(0.95): evaluated on the device from the result still held in HBM (calcMMt.R:13)
    out, _ = rcpp_api.last_mmt_normalised(MMt.shape[0], device=device)
    return out


def calculate_a_and_vara(geno, maxmemGb=8, selectedloci=np.nan, invMMtsqrt=None, transformed_a=None,
                         transformed_vara=None, quiet=True, message=None, device=0):
    fnameMt = geno["asciifileMt"]
    dimsMt = (geno["dim_of_ascii_M"][1], geno["dim_of_ascii_M"][0])  # calculate_a_and_vara.R:21
    return rcpp_api.calculate_a_and_vara_rcpp(f_name_ascii=fnameMt, selected_loci=_shift_if_no_na(selectedloci),
                                              inv_MMt_sqrt=invMMtsqrt, dim_reduced_vara=transformed_vara,
                                              max_memory_in_Gbytes=maxmemGb, dims=dimsMt, a=transformed_a, quiet=quiet,
                                              message=message, device=device)


def extract_geno(fnameM, colnum, availmemGb=8, dim_of_ascii_M=None, device=0):
    """E/R/extract_geno.R:1-19 (colnum is 1-based; the C++ side is 0-based)."""
    return rcpp_api.extract_geno_rcpp(f_name_ascii=fnameM, max_memory_in_Gbytes=availmemGb, selected_locus=colnum - 1,
                                      dims=dim_of_ascii_M, device=device)


def check_for_NA_in_trait(trait):
    """check_for_NA_in_trait.R:1-25: the 1-based positions of NA (NaN) in trait, largest first, or an empty array."""
    idx = np.flatnonzero(np.isnan(np.asarray(trait, dtype=np.float64).ravel())) + 1
    return idx[::-1].copy()


def ReshapeM(fnameM, fnameMt, indxNA, dims, view=False, device=0):
    """ReshapeM.R:1-11: indxNA is 1-based (R), the C++ side 0-based.  Returns the new dims of M (lines, length of the last line).
    view=True: no files are written; fnameM + "tmp" and fnameMt + "tmp" become views on `device`'s context."""
    return rcpp_api.ReshapeM_rcpp(fnameM=fnameM, fnameMt=fnameMt, indxNA=np.asarray(indxNA, dtype=np.int64) - 1, dims=dims, view=view,
                                  device=device)


def constructX(fnameM, currentX, loci_indx, availmemGb=8, dim_of_ascii_M=None, device=0):
    """E/R/constructX.R:1-24 (column names are the R caller's business)."""
    if loci_indx is None or (isinstance(loci_indx, float) and np.isnan(loci_indx)):
        return currentX
    g = extract_geno(fnameM, int(loci_indx), availmemGb, dim_of_ascii_M, device=device)
    return np.column_stack([currentX, g.astype(np.float64)])


def ReadZmat(filename=None, message=None):
    """E/R/ReadZmat.R:34-111: the Z matrix of a repeated-measures design from a whitespace table of 0 and 1, one row per record and
    one column per genotyped individual, every row holding exactly one 1.  Returns the dense n_obs x n_ind matrix (the reference's
    return type; zmat_index turns it into the vector everything else takes), or None after the reference's messages."""
    say = message or (lambda s: None)

    def fail(*lines):
        for ln in ("  ",) + lines + ("   ", "        ReadZmat has terminated with errors.", " "):
            say(ln)
        return None

    if filename is None or not os.path.exists(filename):
        say(" The marker file %s could not be found. " % filename)
        say(" ReadZmat has terminated with errors.")
        return None
    with open(filename) as f:
        rows = [ln.split() for ln in f if ln.strip()]
    try:
        Z = np.array([[float(v) for v in r] for r in rows], dtype=np.float64)
    except ValueError:
        Z = None
    if Z is None or Z.ndim != 2 or Z.dtype == object or not np.isin(Z, (0.0, 1.0)).all():
        return fail(" ERROR: The Z matrix file contains values other than 0 and 1.")
    rs = Z.sum(axis=1)
    if np.any(rs == 0):
        return fail(" ERROR:  The rows %s in the Z matrix have only 0 values." % " ".join(str(i + 1) for i in np.flatnonzero(rs == 0)),
                    "         Each row must contain a single 1 value. ")
    if np.any(rs != 1):
        return fail(" ERROR:  The rows %s in the Z matrix are incorrect." % " ".join(str(i + 1) for i in np.flatnonzero(rs != 1)),
                    "         A row can only contains 0s and a single 1. ")
    say("\n\n Loading Z matrix file ... \n\n")
    say("                    Summary of Z matrix File  \n")
    say("                   ~~~~~~~~~~~~~~~~~~~~~~~~~~~~ \n")
    say(" File name:                   %s\n" % os.path.abspath(filename))
    say(" Number of rows:              %d\n" % Z.shape[0])
    say(" Number of columns:           %d\n" % Z.shape[1])
    return Z


def zmat_index(Zmat):
    """ind_of_obs: for every row of a Z matrix the 0-based column of its 1 (int64).  The form AM(Zmat=), emma_*(Z=) and
    host_model.scan_operands_z work on: n_obs numbers instead of n_obs x n_ind."""
    Z = np.asarray(Zmat)
    if Z.ndim != 2 or not np.isin(Z, (0, 1)).all() or not np.all(Z.sum(axis=1) == 1):
        raise ValueError("a Z matrix holds 0 and 1 with exactly one 1 in every row")
    return np.argmax(Z, axis=1).astype(np.int64)


def find_qtl(geno, availmemGb, selected_loci, MMt, invMMt, best_ve, best_vg, currentX, ncpu, quiet, trait, ngpu=1,
             device=0, return_stats=False, Zmat=None):
    """E/R/find_qtl.R:1-84.  Host algebra (H, P, MMt^{+-1/2}, a_hat, Var a_hat) on host LAPACK, the genome scan and
    the arg-max on the GPU.  Returns the 1-based column of the selected marker.
    Zmat (not in the reference's .find_qtl): the repeated-measures design as ind_of_obs, the dense matrix or a host_model.ZModel
    kept by the caller; trait and currentX then have one row per record, MMt one per individual, and S, V, a_hat come from
    host_model.scan_operands_z (invMMt is not used)."""
    if Zmat is not None:
        zm = Zmat if isinstance(Zmat, host_model.ZModel) else None
        if zm is None:
            from . import am
            Zmat = am.as_ind_of_obs(Zmat)
        op = host_model.scan_operands_z(MMt, Zmat, currentX, trait, best_ve, best_vg, zmodel=zm)
        sq = {"inverse_sqrt_MMt": op["S"]}
        hat_a, var_hat_a = op["ahat"], op["V"]
    else:
        H = host_model.calculateH(MMt, best_ve, best_vg)
        P = host_model.calculateP(H, currentX)
        sq = host_model.calculateMMt_sqrt_and_sqrtinv(MMt, checkres=not quiet)
        hat_a = host_model.calculate_reduced_a(best_vg, P, sq["sqrt_MMt"], trait)
        var_hat_a = host_model.calculate_reduced_vara(currentX, best_ve, best_vg, invMMt, sq["sqrt_MMt"])
    a_and_vara = calculate_a_and_vara(geno=geno, maxmemGb=availmemGb, selectedloci=selected_loci,
                                      invMMtsqrt=sq["inverse_sqrt_MMt"], transformed_a=hat_a,
                                      transformed_vara=var_hat_a, quiet=quiet, device=device)
    indx, tsqmax, near = rcpp_api.last_scan_argmax(device=device)  # find_qtl.R:71-83 on the device
    if return_stats:
        return indx, {"tsqmax": tsqmax, "near_ties": near, "a": a_and_vara["a"], "vara": a_and_vara["vara"]}
    return indx


def create_ascii(file_genotype, type="text", AA=None, AB=None, BB=None, availmemGb=8, dim_of_ascii_M=None, quiet=True,
                 missing=None, outdir=None, message=None, device=0):
    """E/R/create_ascii.R:1-62 -> True / False; writes <outdir>/M.ascii and <outdir>/Mt.ascii (R: tempdir())."""
    outdir = outdir or os.path.dirname(os.path.abspath(file_genotype))
    asciiMfile, asciiMtfile = os.path.join(outdir, "M.ascii"), os.path.join(outdir, "Mt.ascii")
    dims = [int(dim_of_ascii_M[0]), int(dim_of_ascii_M[1])]
    if type == "text":
        missing = "NA" if missing is None else str(missing)                       # :30-34
        if not rcpp_api.createM_ASCII_rcpp(file_genotype, asciiMfile, type, AA, AB, BB, availmemGb, dims, quiet, message, missing,
                                           device=device):
            return False
        rcpp_api.createMt_ASCII_rcpp(asciiMfile, asciiMtfile, type, availmemGb, dims, quiet, message, device=device)
    else:
        ncol = dims[1]
        dims[1] = 2 * dims[1] + 6                                                   # :46-47 columns of a PLINK ped file
        if not rcpp_api.createM_ASCII_rcpp(file_genotype, asciiMfile, type, "-9", "-9", "-9", availmemGb, dims, quiet, message, "NA",
                                           device=device):
            return False
        dims[1] = ncol                                                              # :54
        rcpp_api.createMt_ASCII_rcpp(asciiMfile, asciiMtfile, type, availmemGb, dims, quiet, message, device=device)
    return True


def _count_lines(path):
    """Lines of a text file as getline() counts them: an unterminated tail is a line too."""
    lines, last = 0, b"\n"
    with open(path, "rb") as f:
        for buf in iter(lambda: f.read(1 << 24), b""):
            lines += buf.count(b"\n")
            last = buf[-1:]
    return lines + (last != b"\n")


def bed_fileset(filename):
    """(.bed, .bim, .fam) paths of a PLINK binary fileset named by its .bed file or by the common prefix."""
    prefix = filename[:-4] if str(filename).lower().endswith(".bed") else str(filename)
    return prefix + ".bed", prefix + ".bim", prefix + ".fam"


def ReadBim(path):
    """The marker map of a PLINK .bim file (chromosome, name, genetic distance, position, allele 1, allele 2 per line) ->
    {"SNP": names, "Chr": chromosomes, "Pos": base-pair positions}: usable as map= of SummaryAM / SummaryAM_traits."""
    out = {"SNP": [], "Chr": [], "Pos": []}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            t = line.split()
            if not t:
                continue
            if len(t) < 4:
                raise ValueError("%s line %d: a .bim line has 6 fields, found %d" % (path, ln, len(t)))
            out["Chr"].append(t[0])
            out["SNP"].append(t[1])
            out["Pos"].append(int(t[3]))
    return out


def _read_marker_bed(filename, availmemGb, quiet, outdir, message, device):
    say = message or (lambda s: None)
    files = bed_fileset(filename) if filename is not None else (None,) * 3
    for f, what in zip(files, ("PLINK bed", "PLINK bim", "PLINK fam")):
        if f is None or not os.path.exists(f):
            say(" The %s file %s could not be found. " % (what, f))
            say(" ReadMarker has terminated with errors ")
            return None
    bed, bim, fam = (os.path.abspath(f) for f in files)
    outdir = outdir or os.path.dirname(bed)
    say(" Getting number of individuals and snp from file ... ")
    dims = [_count_lines(fam), _count_lines(bim)]
    say(" Beginning creation of reformatted file ... ")
    asciiM, asciiMt = os.path.join(outdir, "M.ascii"), os.path.join(outdir, "Mt.ascii")
    rcpp_api.create_ascii_from_bed(bed, asciiM, asciiMt, availmemGb, dims, quiet, message, device=device)
    return {"asciifileM": asciiM, "asciifileMt": asciiMt, "dim_of_ascii_M": dims}


# ---- VCF ingestion (include/eagle_hip.h section 1b-vcf): the restatement in plain Python and numpy, and the interface ----
_VCF_COUNT_FIELDS = ("lines", "kept", "multiallelic", "no_alt", "no_gt", "not_snp", "filtered", "missing", "haploid", "malformed")


def _vcf_gt(field):
    """One sample field -> (class, haploid, malformed): class 0 homozygous REF, 1 het, 2 homozygous ALT, -1 missing (rule 4)."""
    tokens = field.split(b":", 1)[0].replace(b"|", b"/").split(b"/")
    if all(t in (b"0", b"1") for t in tokens):
        if len(tokens) == 1:
            return (2 if tokens[0] == b"1" else 0), 1, 0
        if len(tokens) == 2:
            return (tokens[0] == b"1") + (tokens[1] == b"1"), 0, 0
    return -1, 0, int(any(t != b"." for t in tokens))


def vcf_to_bed_host(vcf_bytes, a2="ref", snps_only=False, pass_only=False):
    """eagle_vcf_to_bed restated in plain Python and numpy from the rule of include/eagle_hip.h section 1b-vcf: the bytes of a plain-text
    VCF file -> (bed_bytes, bim_text, fam_text, dims, counts), what the call leaves in <prefix>.bed / .bim / .fam, dims = [n, kept
    markers] and the counts as a dict.  ValueError, with the 1-based line number where the rule gives one, where the call fails.  Host
    only, one Python step per sample field: for tests and small files."""
    if a2 not in ("ref", "alt"):
        raise ValueError('vcf_to_bed_host: a2 must be "ref" or "alt"')
    lines = bytes(vcf_bytes).split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                            # the bytes behind the last '\n' are a line only when there are some
    names, rows, bim = None, [], []
    counts = dict.fromkeys(_VCF_COUNT_FIELDS, 0)
    # the .bed code of a class: by default A1 = ALT, so homozygous REF is hom A2 = 3; a2="alt" turns the two homozygotes round
    code_of = {0: 0 if a2 == "alt" else 3, 1: 2, 2: 3 if a2 == "alt" else 0, -1: 1}
    seen = {}
    for ln, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line or line.startswith(b"##"):
            continue
        col = line.split(b"\t")
        if names is None:
            if not line.startswith(b"#CHROM"):
                raise ValueError("line %d: no #CHROM line in front of the data" % ln)
            if len(col) < 10:
                raise ValueError("line %d: the #CHROM line has fewer than 10 columns" % ln)
            names = col[9:]
            if any(s == b"" or b" " in s for s in names):
                raise ValueError("line %d: a sample name that is empty or contains a blank" % ln)
            continue
        counts["lines"] += 1
        if len(col) < 9:
            raise ValueError("line %d: a data line with fewer than nine fixed fields" % ln)
        chrom, pos, vid, ref, alt, _, flt, _, fmt = col[:9]
        if b"," in alt:
            counts["multiallelic"] += 1
        elif alt == b".":
            counts["no_alt"] += 1
        elif not (fmt == b"GT" or fmt.startswith(b"GT:")):
            counts["no_gt"] += 1
        elif snps_only and not (ref.upper() in (b"A", b"C", b"G", b"T") and alt.upper() in (b"A", b"C", b"G", b"T")):
            counts["not_snp"] += 1
        elif pass_only and flt not in (b"PASS", b"."):
            counts["filtered"] += 1
        else:
            fields = col[9:]
            if len(fields) != len(names):
                raise ValueError("line %d: %d sample fields, the header names %d" % (ln, len(fields), len(names)))
            row = np.empty(len(names), dtype=np.uint8)
            for i, f in enumerate(fields):
                g = seen.get(f)
                if g is None:
                    g = seen[f] = _vcf_gt(f)
                row[i] = code_of[g[0]]
                counts["missing"] += g[0] < 0
                counts["haploid"] += g[1]
                counts["malformed"] += g[2]
            rows.append(row)
            a1, a2_allele = (ref, alt) if a2 == "alt" else (alt, ref)
            bim.append(b"\t".join((chrom, chrom + b":" + pos if vid == b"." else vid, b"0", pos, a1, a2_allele)))
            counts["kept"] += 1
    if names is None:
        raise ValueError("line %d: no #CHROM line" % (len(lines) + 1))
    if not rows:
        raise ValueError("no data line is kept, so there is no fileset to write")
    bed = b"\x6c\x1b\x01" + pack_bed_codes(np.stack(rows)).tobytes()
    bim_text = b"".join(b + b"\n" for b in bim).decode("latin-1")
    fam_text = b"".join(s + b" " + s + b" 0 0 0 -9\n" for s in names).decode("latin-1")
    return bed, bim_text, fam_text, [len(names), len(rows)], {k: int(v) for k, v in counts.items()}


def VcfToBed(vcf, out_prefix, a2="ref", snps_only=False, pass_only=False, availmemGb=8, chunk_bytes=0, device=0):
    """A VCF 4.x file as the PLINK binary fileset out_prefix + ".bed" / ".bim" / ".fam" (rcpp_api.vcf_to_bed: the GT fields are decoded
    on the device, a missing call stays missing) -> {"bed", "bim", "fam", "dims", "counts", "samples"}.  A path that ends in .gz or
    .bgz is first inflated with the standard library's gzip (a bgzip file is a multi-member gzip file) into a scratch file beside the
    output, removed afterwards.  a2="ref" (default): A1 = ALT, A2 = REF, the PLINK program's import convention as documented;
    a2="alt": the library's '2' allele counts ALT copies.  Agreement with PLINK or bcftools is neither claimed nor tested."""
    import gzip
    import shutil
    vcf, prefix = os.fspath(vcf), os.fspath(out_prefix)
    if not os.path.exists(vcf):
        raise ValueError("VcfToBed: the file %s could not be found" % vcf)
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    scratch = None
    try:
        if vcf.lower().endswith((".gz", ".bgz")):
            scratch = prefix + ".inflated.vcf"
            with gzip.open(vcf, "rb") as src, open(scratch, "wb") as dst:
                shutil.copyfileobj(src, dst, 1 << 24)
        res = rcpp_api.vcf_to_bed(scratch or vcf, prefix, a2=a2, snps_only=snps_only, pass_only=pass_only, availmemGb=availmemGb,
                                  chunk_bytes=chunk_bytes, device=device)
    finally:
        if scratch is not None and os.path.exists(scratch):
            os.remove(scratch)
    with open(res["fam"]) as f:
        res["samples"] = [ln.split()[0] for ln in f if ln.strip()]
    return res


def ReadMarker(filename=None, type="text", missing=None, AA=None, AB=None, BB=None, availmemGb=16, quiet=True, outdir=None,
               message=None, device=0, maf=None, max_missing=None, drop_monomorphic=False, impute=None, impute_local=None,
               impute_ld_from="panel", vcf_a2="ref", vcf_snps_only=False, vcf_pass_only=False):
    """E/R/ReadMarker.R:194-318 -> geno dict {asciifileM, asciifileMt, dim_of_ascii_M} or None (the R list / NULL).
    type="PLINKbed" (not in the reference): `filename` is the .bed file of a PLINK binary fileset or its prefix; n and L are the
    line counts of the .fam and .bim beside it, the genotypes go through rcpp_api.create_ascii_from_bed.
    maf / max_missing / drop_monomorphic (not in the reference; all off by default, and then nothing here differs from the line
    above): the converted panel goes through FilterMarkers -- with the .bed file's own counts for type="PLINKbed", so that
    missingness is the file's, not the heterozygotes it became -- into <outdir>/qc, and the dict returned names those files and
    carries marker_index (None when no marker passes).
    impute=k (not in the reference; type="PLINKbed" only; default None, and then nothing here differs from the lines above): after the
    ingestion the missing genotypes of the fileset are filled by ImputeBed(k=k) into <outdir>/imputed/panel.bed / .bim / .fam, that
    fileset is ingested into <outdir>/imputed, and the dict returned names ITS files.  With a filter as well, the imputed panel is
    filtered, on the statistics of the original file's called genotypes.
    impute_local=l (with impute=k; default None, and then nothing here differs from the lines above): ImputeBed(k=k, local=l), LD-kNNi
    with the chromosomes of the fileset's .bim file.  impute_ld_from="bed" (default "panel": nothing differs) passes ld_from="bed": the
    partners in local LD come from the .bed file's own pairwise-complete r2.
    type="VCF" (not in the reference): `filename` is a VCF 4.x file, plain or .gz / .bgz.  VcfToBed converts it into
    <outdir>/vcf/panel.bed / .bim / .fam (vcf_a2, vcf_snps_only, vcf_pass_only are its a2, snps_only, pass_only), and that prefix goes
    through the type="PLINKbed" route above with the caller's maf, max_missing, drop_monomorphic, impute, impute_local and
    impute_ld_from: everything downstream is the .bed route's own code.  The dict returned gains "bed" (the prefix to pass as bed= to
    MarkerStats, Relatedness, LDPrune, ...: the missing calls of the VCF are still missing there), "samples" and "vcf_counts"."""
    say = message or (lambda s: None)
    if type == "VCF":
        if filename is None or not os.path.exists(filename):
            say(" The VCF file %s could not be found. " % filename)
            say(" ReadMarker has terminated with errors ")
            return None
        outdir = outdir or os.path.dirname(os.path.abspath(filename))
        say(" Converting the VCF file into a PLINK binary fileset ... ")
        res = VcfToBed(filename, os.path.join(outdir, "vcf", "panel"), a2=vcf_a2, snps_only=vcf_snps_only, pass_only=vcf_pass_only,
                       availmemGb=availmemGb, device=device)
        prefix = res["bed"][:-4]
        geno = ReadMarker(prefix, type="PLINKbed", availmemGb=availmemGb, quiet=quiet, outdir=outdir, message=message, device=device, maf=maf,
                          max_missing=max_missing, drop_monomorphic=drop_monomorphic, impute=impute, impute_local=impute_local,
                          impute_ld_from=impute_ld_from)
        if geno is None:
            return None
        geno = dict(geno)
        geno.update(bed=prefix, samples=res["samples"], vcf_counts=res["counts"])
        return geno
    if impute is not None and type != "PLINKbed":
        say(' impute needs type = "PLINKbed": only a .bed file still knows which genotypes are missing. \n')
        say(" ReadMarker has terminated with errors")
        return None
    if maf is not None or max_missing is not None or drop_monomorphic:
        geno = ReadMarker(filename, type=type, missing=missing, AA=AA, AB=AB, BB=BB, availmemGb=availmemGb, quiet=quiet, outdir=outdir,
                          message=message, device=device, impute=impute, impute_local=impute_local, impute_ld_from=impute_ld_from)
        if geno is None:
            return None
        return FilterMarkers(geno, maf=maf, max_missing=max_missing, drop_monomorphic=drop_monomorphic,
                             bed=bed_fileset(filename)[0] if type == "PLINKbed" else None, availmemGb=availmemGb, message=message, device=device)
    if type == "PLINKbed":
        geno = _read_marker_bed(filename, availmemGb, quiet, outdir, message, device)
        if geno is None or impute is None:
            return geno
        imputed = os.path.join(os.path.dirname(geno["asciifileM"]), "imputed")
        if impute_local is None:
            res = ImputeBed(filename, geno, os.path.join(imputed, "panel"), k=int(impute), availmemGb=availmemGb, message=message, device=device)
        else:
            res = ImputeBed(filename, geno, os.path.join(imputed, "panel"), k=int(impute), availmemGb=availmemGb, message=message, device=device,
                            local=int(impute_local), map=ReadBim(bed_fileset(filename)[1]), ld_from=impute_ld_from)
        return _read_marker_bed(res["bed"], availmemGb, quiet, imputed, message, device)
    if type not in ("text", "PLINK"):                                               # :206-215
        say(' type must be set to "text" or "PLINK". \n')
        say(" ReadMarker has terminated with errors")
        return None
    if filename is None or not os.path.exists(filename):                            # :222-231, check_inputs.R
        say(" The %s file %s could not be found. " % ("PLINK ped" if type == "PLINK" else "marker", filename))
        say(" ReadMarker has terminated with errors ")
        return None
    genofile = os.path.abspath(filename)
    outdir = outdir or os.path.dirname(genofile)
    if type == "PLINK":
        dims = rcpp_api.getRowColumn(genofile, device=device)                       # :234-235
        dims[1] = (dims[1] - 6) // 2
        ok = create_ascii(genofile, type=type, availmemGb=availmemGb, dim_of_ascii_M=dims, quiet=quiet, outdir=outdir,
                          message=message, device=device)
    else:
        if AA is None or BB is None:                                                # :262-268
            say("Error: The function parameters AA and BB must be assigned a numeric or character value since a text file is being assumed. \n")
            say(" ReadMarker has terminated with errors")
            return None
        if AB is None:
            AB = "NA"                                                               # :271-272 no hets
        say(" Getting number of individuals and snp from file ... ")
        dims = rcpp_api.getRowColumn(genofile, device=device)                       # :283
        say(" Beginning creation of reformatted file ... ")
        ok = create_ascii(genofile, type=type, AA=str(AA), AB=str(AB), BB=str(BB), availmemGb=availmemGb, dim_of_ascii_M=dims,
                          quiet=quiet, missing=missing, outdir=outdir, message=message, device=device)
    if not ok:
        return None
    return {"asciifileM": os.path.join(outdir, "M.ascii"), "asciifileMt": os.path.join(outdir, "Mt.ascii"), "dim_of_ascii_M": dims}


# ---- kNN imputation of a PLINK .bed fileset (include/eagle_hip.h section 1b'''i): the restatements in numpy and the interface ----
KNN_MAX_K = 256
_DOSAGE_OF_CODE = np.array([0, 0, 1, 2], dtype=np.int64)     # 2-bit code -> dosage (code 1, missing, has none)
_CODE_OF_DOSAGE = np.array([0, 2, 3], dtype=np.uint8)


def read_bed_codes(bed, dims):
    """The 2-bit codes of a SNP-major .bed file (or fileset prefix) -> uint8 (L, n): 0 hom A1, 1 missing, 2 het, 3 hom A2.  Host only."""
    n, L = int(dims[0]), int(dims[1])
    rb = (n + 3) // 4
    raw = np.fromfile(bed_fileset(bed)[0], dtype=np.uint8)
    if raw.size != 3 + L * rb or bytes(raw[:3]) != b"\x6c\x1b\x01":
        raise ValueError("%s is not a SNP-major .bed file of %d markers of %d individuals" % (bed, L, n))
    rows = raw[3:].reshape(L, rb)
    return np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(L, 4 * rb)[:, :n].copy()


def pack_bed_codes(codes):
    """uint8 (L, n) 2-bit codes -> uint8 (L, ceil(n/4)): the rows of a SNP-major .bed file, pad bit pairs 00."""
    codes = np.asarray(codes, dtype=np.uint8)
    L, n = codes.shape
    f = np.zeros((L, (n + 3) // 4 * 4), dtype=np.uint8)
    f[:, :n] = codes
    f = f.reshape(L, -1, 4)
    return (f[:, :, 0] | f[:, :, 1] << 2 | f[:, :, 2] << 4 | f[:, :, 3] << 6).astype(np.uint8)


def knn_distance(ibs0, hethet):
    """d_ij = 4 ibs0_ij + h_i + h_j - 2 hethet_ij, h = diag(hethet), -> int32 (n, n): the sum over the markers of (g_i - g_j)^2 for
    g in {-1, 0, +1}, from rcpp_api.sample_ibs' matrices (int32 arithmetic as on the device: exact while 4 L < 2^31)."""
    a, hh = np.asarray(ibs0, dtype=np.int64), np.asarray(hethet, dtype=np.int64)
    h = np.diagonal(hh)
    return (4 * a + h[:, None] + h[None, :] - 2 * hh).astype(np.int32)


def knn_rows_host(d, K):
    """rcpp_api.knn_rows restated in numpy: d = knn_distance(...) -> int32 (n, K).  Row i = the min(K, n - 1) individuals j != i with
    the smallest keys (uint64)(uint32)d_ij << 32 | j in increasing order, then -1."""
    d = np.asarray(d, dtype=np.int32)
    n, K = d.shape[0], int(K)
    if d.shape != (n, n) or not 1 <= K <= KNN_MAX_K:
        raise ValueError("knn_rows_host: d must be square and K in [1, %d]" % KNN_MAX_K)
    keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    np.fill_diagonal(keys, np.iinfo(np.uint64).max)
    keff = min(K, n - 1)
    out = np.full((n, K), -1, dtype=np.int32)
    if keff:
        part = np.partition(keys, keff - 1, axis=1)[:, :keff] if keff < n - 1 else keys
        out[:, :keff] = (np.sort(part, axis=1)[:, :keff] & np.uint64(0xffffffff)).astype(np.int32)
    return out


def impute_knn_host(codes, nbr, k, min_votes):
    """rcpp_api.bed_impute_knn restated in numpy: codes = uint8 (L, n) 2-bit codes of the input (read_bed_codes), nbr = int32 (n, K)
    -> (rows, counts): rows = uint8 (L, ceil(n/4)), the marker rows of the output .bed file (everything after its three header bytes),
    counts = int32 (L, 2), genotypes imputed by vote and by fallback.  The rule is the header's: the first k neighbours of the list
    that are called at the marker vote, the dosage is (2 s + c) // (2 c), and with fewer than min_votes voters the marker's own calls
    give it (heterozygous when it has none)."""
    codes = np.asarray(codes, dtype=np.uint8)
    nbr = np.asarray(nbr, dtype=np.int64)
    L, n = codes.shape
    k, min_votes = int(k), int(min_votes)
    if nbr.ndim != 2 or nbr.shape[0] != n or not 1 <= nbr.shape[1] <= KNN_MAX_K or not 1 <= k <= nbr.shape[1] or min_votes < 1:
        raise ValueError("impute_knn_host: nbr must be (n, K), 1 <= K <= %d, 1 <= k <= K, min_votes >= 1" % KNN_MAX_K)
    if nbr.size and (nbr.min() < -1 or nbr.max() >= n):
        raise ValueError("impute_knn_host: a neighbour outside [-1, n)")
    miss = codes == 1
    c = np.zeros((L, n), dtype=np.int64)
    s = np.zeros((L, n), dtype=np.int64)
    for t in range(nbr.shape[1]):
        j = nbr[:, t]
        cj = codes[:, np.maximum(j, 0)]                             # (L, n): the code of i's t-th neighbour at every marker
        vote = miss & (j >= 0)[None, :] & (cj != 1) & (c < k)
        c += vote
        s += np.where(vote, _DOSAGE_OF_CODE[cj], 0)
    called = (~miss).sum(axis=1)
    dose = np.where(miss, 0, _DOSAGE_OF_CODE[codes]).sum(axis=1)
    fb = np.where(called > 0, _CODE_OF_DOSAGE[(2 * dose + called) // np.maximum(2 * called, 1)], 2).astype(np.uint8)
    by_vote = miss & (c >= min_votes)
    voted = _CODE_OF_DOSAGE[np.where(by_vote, (2 * s + c) // np.maximum(2 * c, 1), 0)]
    out = np.where(by_vote, voted, np.where(miss, fb[:, None], codes)).astype(np.uint8)
    counts = np.stack([by_vote.sum(axis=1), (miss & ~by_vote).sum(axis=1)], axis=1).astype(np.int32)
    return pack_bed_codes(out), counts


DIST_NO_OVERLAP = 0xFFFFFFFE


def _bed_include_mask(include, L, who):
    """None, a bool mask of length L or a list of 0-based marker indices -> None or a bool mask of length L."""
    if include is None:
        return None
    a = np.atleast_1d(np.asarray(include)).ravel()
    if a.dtype == bool:
        if a.size != L:
            raise ValueError("%s: the include mask holds %d entries, the .bed file %d markers" % (who, a.size, L))
        return a.copy()
    idx = a.astype(np.int64)
    if not np.array_equal(idx, a) or (idx.size and (idx.min() < 0 or idx.max() >= L)):
        raise ValueError("%s: include must be a bool mask or whole marker indices in [0, %d)" % (who, L))
    m = np.zeros(L, dtype=bool)
    m[idx] = True
    return m


def bed_ibs_host(codes, include=None, min_overlap=1):
    """rcpp_api.bed_sample_ibs restated in numpy (include/eagle_hip.h section 1b'''ii): codes = uint8 (L, n) 2-bit codes (read_bed_codes),
    include = None, a bool mask of length L or marker indices -> (ncalled, ibs0, hethet, hetsum, dist), int32 (n, n) x 4 and uint32
    (n, n).  g = -1, 0, 0, +1, u = |g|, h = [code == 2], c = [code != 1] per genotype, zero at excluded markers; D = g g^T, Q = u u^T,
    H = h h^T, N = c c^T; ncalled = N, ibs0 = (Q - D) / 2, hethet = H, hetsum = H + N - Q; dist = (4 ibs0 + hetsum - 2 hethet) * Linc
    // N, DIST_NO_OVERLAP where N < min_overlap."""
    codes = np.asarray(codes, dtype=np.uint8)
    L = codes.shape[0]
    min_overlap = int(min_overlap)
    if min_overlap < 1:
        raise ValueError("bed_ibs_host: min_overlap must be at least 1")
    inc = _bed_include_mask(include, L, "bed_ibs_host")
    if inc is not None:
        codes = codes[inc]
    linc = codes.shape[0]
    g = np.array([-1.0, 0.0, 0.0, 1.0])[codes]            # fp64 products of 0 / +-1 summed over L < 2^53 markers: exact integers
    u, h, c = np.abs(g), (codes == 2).astype(np.float64), (codes != 1).astype(np.float64)
    D, Q, H, N = (np.rint(x.T @ x).astype(np.int64) for x in (g, u, h, c))
    ibs0, hetsum = (Q - D) // 2, H + N - Q
    d = 4 * ibs0 + hetsum - 2 * H
    dist = np.where(N >= min_overlap, d * linc // np.maximum(N, 1), DIST_NO_OVERLAP).astype(np.uint32)
    return N.astype(np.int32), ibs0.astype(np.int32), H.astype(np.int32), hetsum.astype(np.int32), dist


# ---- LD-kNNi (include/eagle_hip.h section 1b'''iii): the restatements in numpy ----
LDKNN_MAX_PARTNERS = 32
LDKNN_MAX_K = 64


def ld_band_host(Mt8, window):
    """The fp64 r2 band of the ingested panel (include/eagle_hip.h section 1b'''iii) in numpy: Mt8 = int8 (L, n) marker-major genotypes
    in {-1, 0, +1} -> fp64 (L, window), band[i, o - 1] = r2 between markers i and i + o = fl(fl((double)c * (double)c) / fl((double)v_i *
    (double)v_j)), -1.0 where i + o >= L or one of the two is monomorphic: what k_ld_tile's r2 mode writes."""
    G = np.asarray(Mt8)
    L, n = G.shape
    window = int(window)
    if not 1 <= window <= 256:
        raise ValueError("ld_band_host: 1 <= window <= 256")
    F = G.astype(np.float64)                                   # products and sums of small integers: exact in fp64 below 2^53
    Gi = G.astype(np.int64)
    s, q = Gi.sum(axis=1), (Gi * Gi).sum(axis=1)
    v = n * q - s * s
    vf = v.astype(np.float64)
    band = np.full((L, window), -1.0)                          # band[i, o - 1] = r2 between i and i + o, -1.0 without one
    for o in range(1, min(window, L - 1) + 1):
        d = np.rint(np.einsum("ij,ij->i", F[:-o], F[o:])).astype(np.int64)          # markers i = 0 .. L - o - 1 with j = i + o
        c = (n * d - s[:-o] * s[o:]).astype(np.float64)
        ok = (v[:-o] > 0) & (v[o:] > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            r2 = (c * c) / (vf[:-o] * vf[o:])
        band[:-o, o - 1] = np.where(ok, r2, -1.0)
    return band


def ld_partners_host(Mt8, window, l, min_r2, chrom=None):
    """rcpp_api.ld_partners restated in numpy: Mt8 = int8 (L, n) marker-major genotypes in {-1, 0, +1} (the ingested panel: missing
    genotypes are heterozygotes) -> (partners int32 (L, l), r2 fp64 (L, l)).  r2_ij = fl(fl((double)c * (double)c) / fl((double)v_i *
    (double)v_j)) for v_i, v_j > 0; row i lists the j with 1 <= |j - i| <= window, r2_ij >= min_r2 and chrom[j] == chrom[i] by
    decreasing r2, ties to the smaller |j - i|, then the smaller j; -1 (r2 0.0) beyond them."""
    G = np.asarray(Mt8)
    L, n = G.shape
    window, l, min_r2 = int(window), int(l), float(min_r2)
    if not 1 <= window <= 256 or not 1 <= l <= LDKNN_MAX_PARTNERS or not 0.0 <= min_r2 <= 1.0:
        raise ValueError("ld_partners_host: 1 <= window <= 256, 1 <= l <= %d, 0 <= min_r2 <= 1" % LDKNN_MAX_PARTNERS)
    ch = None if chrom is None else np.asarray(chrom).ravel()
    if ch is not None and ch.size != L:
        raise ValueError("ld_partners_host: chrom holds %d entries, the panel %d markers" % (ch.size, L))
    band = ld_band_host(G, window)
    return _ld_rank_band(band, l, min_r2, ch)


def _ld_rank_band(band, l, min_r2, ch):
    """The ranking rule of include/eagle_hip.h section 1b'''iii on band[i, o - 1] = r2 between markers i and i + o (-1.0: no pair) ->
    (partners int32 (L, l), r2 fp64 (L, l))."""
    L, window = band.shape
    # column t = 2 (o - 1) + (j > i) holds r2 between i and j = i -+ o: the column index is the rank of a tie
    cols = max(2 * window, l)
    R = np.full((L, cols), -1.0)
    J = np.full((L, cols), -1, dtype=np.int64)
    for o in range(1, min(window, L - 1) + 1):
        r2 = band[:-o, o - 1]
        ok = r2 >= min_r2                                                             # -1.0 is below every min_r2
        if ch is not None:
            ok &= ch[:-o] == ch[o:]
        r2 = np.where(ok, r2, -1.0)
        R[:-o, 2 * (o - 1) + 1] = r2                                                  # forward: j = i + o
        J[:-o, 2 * (o - 1) + 1] = np.arange(o, L)
        R[o:, 2 * (o - 1)] = r2                                                       # backward: the same pair seen from j
        J[o:, 2 * (o - 1)] = np.arange(0, L - o)
    order = np.argsort(-R, axis=1, kind="stable")[:, :l]                              # stable: equal r2 stay in column order
    r2 = np.take_along_axis(R, order, axis=1)
    part = np.take_along_axis(J, order, axis=1)
    return np.where(r2 >= 0.0, part, -1).astype(np.int32), np.where(r2 >= 0.0, r2, 0.0)


# ---- pairwise-complete LD from the .bed file (include/eagle_hip.h section 1b'''iv): the restatements in numpy ----
def bed_ld_host(codes, window, include=None, min_overlap=1):
    """The six sums and r2 of include/eagle_hip.h section 1b'''iv in numpy: codes = uint8 (L, n) 2-bit codes (read_bed_codes), include =
    None, a bool mask of length L or marker indices (the panel) -> (N, D, Si, Sj, Qi, Qj, r2): int64 (Linc, window) x 6 and fp64 (Linc,
    window), entry [i, o - 1] for the panel markers i and j = i + o.  x = -1, 0, 0, +1, c = [code != 1], u = |x|; N = sum c_i c_j,
    D = sum x_i x_j, Si = sum x_i c_j, Sj = sum c_i x_j, Qi = sum u_i c_j, Qj = sum c_i u_j; cov = N D - Si Sj, vi = N Qi - Si^2,
    vj = N Qj - Sj^2; r2 = fl(fl(dc * dc) / fl(dvi * dvj)) where N >= min_overlap, vi > 0 and vj > 0, else -1.0 (and where i + o >= Linc,
    with zero sums)."""
    codes = np.asarray(codes, dtype=np.uint8)
    window, min_overlap = int(window), int(min_overlap)
    if not 1 <= window <= 256 or min_overlap < 1:
        raise ValueError("bed_ld_host: 1 <= window <= 256, min_overlap >= 1")
    inc = _bed_include_mask(include, codes.shape[0], "bed_ld_host")
    if inc is not None:
        codes = codes[inc]
    L = codes.shape[0]
    if L < 1:
        raise ValueError("bed_ld_host: include selects no marker")
    x = np.array([-1.0, 0.0, 0.0, 1.0])[codes]                # fp64 sums of products of 0 / +-1 over n < 2^53 individuals: exact integers
    c, u = (codes != 1).astype(np.float64), np.abs(x)
    out = [np.zeros((L, window), dtype=np.int64) for _ in range(6)]
    r2 = np.full((L, window), -1.0)
    for o in range(1, min(window, L - 1) + 1):
        sums = [np.rint(np.einsum("ij,ij->i", a[:-o], b[o:])).astype(np.int64)
                for a, b in ((c, c), (x, x), (x, c), (c, x), (u, c), (c, u))]
        for dst, v in zip(out, sums):
            dst[:-o, o - 1] = v
        N, D, Si, Sj, Qi, Qj = sums
        cov, vi, vj = N * D - Si * Sj, N * Qi - Si * Si, N * Qj - Sj * Sj
        ok = (N >= min_overlap) & (vi > 0) & (vj > 0)
        dc = cov.astype(np.float64)
        den = np.where(ok, vi.astype(np.float64) * vj.astype(np.float64), 1.0)
        r2[:-o, o - 1] = np.where(ok, (dc * dc) / den, -1.0)
    return (*out, r2)


def bed_ld_mask_host(codes, window, r2, include=None, min_overlap=1):
    """rcpp_api.bed_ld_window restated in numpy -> uint64 (Linc, ceil(window / 64)): bit o - 1 of panel marker i is set iff the pair
    (i, i + o) is comparable and (double)cov * (double)cov > r2 * ((double)vi * (double)vj) (bed_ld_host's sums)."""
    t = np.float64(r2)
    if not 0.0 <= t <= 1.0:
        raise ValueError("bed_ld_mask_host: r2 must be in [0, 1]")
    N, D, Si, Sj, Qi, Qj, _ = bed_ld_host(codes, window, include, min_overlap)
    cov, vi, vj = N * D - Si * Sj, N * Qi - Si * Si, N * Qj - Sj * Sj
    dc = cov.astype(np.float64)
    hit = (N >= int(min_overlap)) & (vi > 0) & (vj > 0) & (dc * dc > t * (vi.astype(np.float64) * vj.astype(np.float64)))
    bits = np.zeros((N.shape[0], (int(window) + 63) // 64 * 64), dtype=np.uint8)
    bits[:, :int(window)] = hit
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").astype(np.uint64)


def bed_ld_partners_host(codes, window, l, min_r2, include=None, min_overlap=1, chrom=None):
    """rcpp_api.bed_ld_partners restated in numpy -> (partners int32 (Linc, l), r2 fp64 (Linc, l)): ld_partners_host's ranking on
    bed_ld_host's r2 band; chrom by panel marker."""
    l, min_r2 = int(l), float(min_r2)
    if not 1 <= l <= LDKNN_MAX_PARTNERS or not 0.0 <= min_r2 <= 1.0:
        raise ValueError("bed_ld_partners_host: 1 <= l <= %d, 0 <= min_r2 <= 1" % LDKNN_MAX_PARTNERS)
    band = bed_ld_host(codes, window, include, min_overlap)[6]
    ch = None if chrom is None else np.asarray(chrom).ravel()
    if ch is not None and ch.size != band.shape[0]:
        raise ValueError("bed_ld_partners_host: chrom holds %d entries, the panel %d markers" % (ch.size, band.shape[0]))
    return _ld_rank_band(band, l, min_r2, ch)


def impute_ldknn_host(codes, partners, k, min_votes, min_overlap):
    """rcpp_api.bed_impute_ldknn restated in numpy: codes = uint8 (L, n) 2-bit codes of the input (read_bed_codes), partners = int32
    (L, l) -> (rows, counts) as impute_knn_host returns them.  For a missing (i, m) the candidates are the j called at m with at least
    min_overlap of m's partners called in both; dist = (d * 4096) // ov over those partners, d = sum (g_i - g_j)^2; the k smallest keys
    dist << 32 | j vote; (2 s + c) // (2 c) with c >= min_votes voters, else the marker's own mean (heterozygous without a call)."""
    codes = np.asarray(codes, dtype=np.uint8)
    P = np.asarray(partners, dtype=np.int64)
    L, n = codes.shape
    k, min_votes, min_overlap = int(k), int(min_votes), int(min_overlap)
    if P.ndim != 2 or P.shape[0] != L or not 1 <= P.shape[1] <= LDKNN_MAX_PARTNERS or not 1 <= k <= LDKNN_MAX_K or min_votes < 1 \
            or not 1 <= min_overlap <= 32:
        raise ValueError("impute_ldknn_host: partners must be (L, l), 1 <= l <= %d, 1 <= k <= %d, min_votes >= 1, 1 <= min_overlap <= 32"
                         % (LDKNN_MAX_PARTNERS, LDKNN_MAX_K))
    if P.size and (P.min() < -1 or P.max() >= L or np.any((P >= 0) & (np.abs(P - np.arange(L)[:, None]) > 256))):
        raise ValueError("impute_ldknn_host: a partner outside [-1, L) or more than 256 rows from its marker")
    gval = np.array([-1.0, 0.0, 0.0, 1.0])
    out = codes.copy()
    counts = np.zeros((L, 2), dtype=np.int32)
    none = np.iinfo(np.uint64).max
    jj = np.arange(n, dtype=np.uint64)
    for m in np.flatnonzero((codes == 1).any(axis=1)):
        row = codes[m]
        I = np.flatnonzero(row == 1)
        called = np.flatnonzero(row != 1)
        fb = _CODE_OF_DOSAGE[(2 * int(_DOSAGE_OF_CODE[row[called]].sum()) + called.size) // (2 * called.size)] if called.size else 2
        Gp = codes[P[m][P[m] >= 0]]                                                  # (partners, n); a repeated partner counts again
        c = (Gp != 1).astype(np.float64)
        g = gval[Gp]
        q = g * g
        ov = np.rint(c[:, I].T @ c).astype(np.int64)                                  # (missing, n)
        d = np.rint(q[:, I].T @ c + c[:, I].T @ q - 2.0 * (g[:, I].T @ g)).astype(np.int64)
        ok = (ov >= min_overlap) & (row != 1)[None, :]
        dist = (d * 4096 // np.maximum(ov, 1)).astype(np.uint64)
        keys = np.where(ok, (dist << np.uint64(32)) | jj[None, :], none)
        keys = np.sort(keys, axis=1)[:, :k]
        voter = keys != none
        cnt = voter.sum(axis=1)
        dose = np.where(voter, _DOSAGE_OF_CODE[row[(keys & np.uint64(0xffffffff)).astype(np.int64) % n]], 0).sum(axis=1)
        by_vote = cnt >= min_votes
        out[m, I] = np.where(by_vote, _CODE_OF_DOSAGE[np.where(by_vote, (2 * dose + cnt) // np.maximum(2 * cnt, 1), 0)], fb)
        counts[m] = (int(by_vote.sum()), int((~by_vote).sum()))
    return pack_bed_codes(out), counts


def _copy_bim_fam(src_bim, out_bim, src_fam, out_fam):
    for src, dst in ((src_bim, out_bim), (src_fam, out_fam)):
        with open(src, "rb") as fi, open(dst, "wb") as fo:
            for buf in iter(lambda: fi.read(1 << 24), b""):
                fo.write(buf)


def ImputeBed(bed, geno, out_prefix, k=10, K=64, min_votes=1, availmemGb=8, message=None, device=0, pairwise=False, min_overlap=1,
              local=None, window=50, min_r2=0.0, local_min_overlap=4, map=None, ld_from="panel", ld_min_overlap=None):
    """kNN imputation of the missing genotypes of a PLINK binary fileset -> {"bed": the new .bed file, "n_missing", "by_vote",
    "by_fallback": totals, "counts": int32 (L, 2) per marker}.  bed = the .bed file (or prefix) that `geno` was ingested from.
    The neighbours come from the ingested panel (rcpp_api.sample_ibs on geno["asciifileM"], knn_distance, rcpp_api.knn_rows: the K
    nearest individuals genome-wide, missing genotypes counted as the heterozygotes ingestion made of them); every missing genotype
    then takes the rounded mean dosage of the first k of them that are called at its marker (rcpp_api.bed_impute_knn; the marker's
    own mean with fewer than min_votes voters).  pairwise=True ranks the neighbours by the .bed file's own pairwise-complete distance
    instead (rcpp_api.bed_sample_ibs, rcpp_api.knn_rows_dist: every pair is compared over the markers where both are called, at
    least min_overlap of them, so shared missingness does not make two individuals look alike).  Writes <out_prefix>.bed and
    byte-for-byte copies of the .bim and .fam; the new fileset has no missing code and ReadMarker(type="PLINKbed") ingests it.
    local=l (default None, and then nothing here differs from the lines above) switches to LD-kNNi (include/eagle_hip.h section
    1b'''iii): every marker's l <= 32 partners in local LD come from the ingested panel (rcpp_api.ld_partners on geno["asciifileMt"]:
    the markers at most `window` away with r2 >= min_r2, on the marker's chromosome when map -- ReadBim's dict -- is given), and a
    missing genotype takes the rounded mean dosage of the k <= 64 individuals called at its marker that are nearest over those
    partners, among the individuals compared over at least local_min_overlap of them (rcpp_api.bed_impute_ldknn).  For panels whose
    members are all about equally related genome-wide (MAGIC, NAM, diversity panels), where the close relative changes from segment
    to segment.  K, pairwise and min_overlap are ignored in this mode; the result carries "partners" as well.
    ld_from="bed" (with local=; default "panel", and then nothing here differs from the lines above) takes the partner lists from the
    input .bed file itself instead, over the whole file: r2 of every pair of markers over the individuals called at both, at least
    ld_min_overlap of them (default max(2, n // 10)) -- rcpp_api.bed_ld_partners, include/eagle_hip.h section 1b'''iv -- so that the
    missing genotypes being imputed do not pull the ranking of the partners towards the heterozygote."""
    say = message or (lambda s: None)
    src_bed, src_bim, src_fam = bed_fileset(bed)
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    out_bed, out_bim, out_fam = bed_fileset(str(out_prefix))
    if os.path.abspath(out_bed) == os.path.abspath(src_bed):
        raise ValueError("ImputeBed: out_prefix names the input fileset")
    if ld_from not in ("panel", "bed"):
        raise ValueError('ImputeBed: ld_from must be "panel" or "bed"')
    if local is not None:
        errs = []
        map = _ld_map("ImputeBed", map, geno, L, errs.append)
        if map is False:
            raise ValueError("ImputeBed:" + errs[0])
        chrom = None if map is None else np.unique(np.asarray([str(c) for c in map["Chr"]]), return_inverse=True)[1].astype(np.int32)
        l = max(1, min(int(local), LDKNN_MAX_PARTNERS))
        k = max(1, min(int(k), LDKNN_MAX_K))
        if ld_from == "bed":
            mo = max(2, n // 10) if ld_min_overlap is None else int(ld_min_overlap)
            partners = rcpp_api.bed_ld_partners(src_bed, (n, L), int(window), l, float(min_r2), None, mo, chrom, availmemGb, device=device)
        else:
            partners = rcpp_api.ld_partners(geno["asciifileMt"], (n, L), int(window), l, float(min_r2), chrom, availmemGb, device=device)
        os.makedirs(os.path.dirname(os.path.abspath(out_bed)), exist_ok=True)
        counts = rcpp_api.bed_impute_ldknn(src_bed, (n, L), partners, k, int(min_votes), int(local_min_overlap), out_bed, availmemGb, device=device)
        _copy_bim_fam(src_bim, out_bim, src_fam, out_fam)
        by_vote, by_fallback = int(counts[:, 0].sum(dtype=np.int64)), int(counts[:, 1].sum(dtype=np.int64))
        say(" Imputed %d missing genotypes: %d from their %d nearest called neighbours over %d markers in local LD, %d from the marker's own mean. "
            % (by_vote + by_fallback, by_vote, k, l, by_fallback))
        return {"bed": out_bed, "n_missing": by_vote + by_fallback, "by_vote": by_vote, "by_fallback": by_fallback, "counts": counts,
                "partners": partners}
    K = max(1, min(int(K), KNN_MAX_K))
    k = max(1, min(int(k), K))
    if pairwise:
        dist = rcpp_api.bed_sample_ibs(src_bed, (n, L), None, int(min_overlap), availmemGb, device=device)[4]
        nbr = rcpp_api.knn_rows_dist(dist, K, device=device)
    else:
        ibs0, hethet = rcpp_api.sample_ibs(geno["asciifileM"], (n, L), availmemGb, device=device)
        nbr = rcpp_api.knn_rows(ibs0, hethet, K, device=device)
    os.makedirs(os.path.dirname(os.path.abspath(out_bed)), exist_ok=True)
    counts = rcpp_api.bed_impute_knn(src_bed, (n, L), nbr, k, int(min_votes), out_bed, availmemGb, device=device)
    _copy_bim_fam(src_bim, out_bim, src_fam, out_fam)
    by_vote, by_fallback = int(counts[:, 0].sum(dtype=np.int64)), int(counts[:, 1].sum(dtype=np.int64))
    say(" Imputed %d missing genotypes: %d from their %d nearest called neighbours, %d from the marker's own mean. "
        % (by_vote + by_fallback, by_vote, k, by_fallback))
    return {"bed": out_bed, "n_missing": by_vote + by_fallback, "by_vote": by_vote, "by_fallback": by_fallback, "counts": counts}


def marker_stats_from_counts(n0, n1, n2, n_missing=None):
    """Per-marker statistics from integer genotype counts, in numpy fp64 (nothing here touches a device): n0 / n1 / n2 = called
    genotypes coded 0 / 1 / 2, n_missing = genotypes without a call (default none).  n = n0 + n1 + n2 + n_missing individuals,
    n_called = n0 + n1 + n2;  freq = (2 n2 + n1) / (2 n_called), the frequency of the allele coded 2;  maf = the smaller of the two
    allele counts over 2 n_called (PLINK's definitions: missing genotypes are in neither);  het = n1 / n_called;  call_rate =
    n_called / n.  A marker without a called genotype has freq = maf = het = NaN and call_rate = 0."""
    n0, n1, n2 = (np.asarray(v, dtype=np.int64).ravel() for v in (n0, n1, n2))
    nm = np.zeros_like(n0) if n_missing is None else np.asarray(n_missing, dtype=np.int64).ravel()
    called = n0 + n1 + n2
    n = called + nm
    a2 = 2 * n2 + n1
    with np.errstate(divide="ignore", invalid="ignore"):
        two = (2 * called).astype(np.float64)
        freq = np.where(called > 0, a2 / two, np.nan)
        maf = np.where(called > 0, np.minimum(a2, 2 * called - a2) / two, np.nan)
        het = np.where(called > 0, n1 / called.astype(np.float64), np.nan)
        call_rate = np.where(n > 0, called / np.maximum(n, 1).astype(np.float64), 0.0)
    return {"n0": n0, "n1": n1, "n2": n2, "n_missing": nm, "freq": freq, "maf": maf, "het": het, "call_rate": call_rate}


def marker_keep_mask(stats, maf=None, max_missing=None, drop_monomorphic=False, hwe=None):
    """Which markers a filter keeps (boolean, length L), by PLINK's rules on the output of marker_stats_from_counts: keep
    maf >= `maf`; drop n_missing / n > `max_missing`; drop_monomorphic drops maf == 0; a marker without a called genotype is dropped
    by any of the three.  hwe drops the markers whose Hardy-Weinberg exact test has p < `hwe` (stats["hwe_p"]: MarkerStats(..., hwe=True)
    or HWE(stats)); it drops nothing else.  With no filter switched on every marker is kept."""
    L = len(stats["n0"])
    keep = np.ones(L, dtype=bool)
    if hwe is not None:
        if "hwe_p" not in stats:
            raise ValueError("marker_keep_mask: hwe= needs stats[\"hwe_p\"] (MarkerStats(..., hwe=True))")
        keep &= ~(np.asarray(stats["hwe_p"], dtype=np.float64) < float(hwe))
    if maf is None and max_missing is None and not drop_monomorphic:
        return keep
    keep &= ~np.isnan(stats["maf"])
    if maf is not None:
        keep &= np.nan_to_num(stats["maf"], nan=-1.0) >= float(maf)
    if max_missing is not None:
        n = stats["n0"] + stats["n1"] + stats["n2"] + stats["n_missing"]
        keep &= ~(stats["n_missing"] / np.maximum(n, 1).astype(np.float64) > float(max_missing))
    if drop_monomorphic:
        keep &= ~(np.nan_to_num(stats["maf"], nan=0.0) == 0.0)
    return keep


def MarkerStats(geno, bed=None, availmemGb=8, device=0, hwe=False):
    """Per-marker QC statistics of a panel -> dict of length-L arrays n0, n1, n2, n_missing, freq, maf, het, call_rate
    (marker_stats_from_counts), with hwe=True also hwe_p, the Hardy-Weinberg exact test of (n0, n1, n2) (HWE); the counting runs on the device (rcpp_api.marker_counts on geno["asciifileMt"]: one pass over the
    int8 image the scans read), the arithmetic on the host.
    The text files of a panel no longer know which genotypes were missing: ingestion made them heterozygotes (unless the fileset went
    through ImputeBed first, which leaves none), so without `bed`
    n_missing is zero, n1 includes them and call_rate is 1.  bed = the .bed file (or prefix) the panel was ingested from: the counts
    are then the file's own (rcpp_api.bed_marker_counts), n0 / n1 / n2 and everything derived exclude the missing genotypes, and
    n_missing is real.  n0 counts the genotype the files code '0' (homozygous A1 of a .bed file)."""
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    if bed is not None:
        c = rcpp_api.bed_marker_counts(bed_fileset(bed)[0], (n, L), availmemGb, device=device)
        stats = marker_stats_from_counts(c[:, 0], c[:, 1], c[:, 2], c[:, 3])
    else:
        c = rcpp_api.marker_counts(geno["asciifileMt"], (n, L), availmemGb, device=device)
        stats = marker_stats_from_counts(c[:, 0], c[:, 1], c[:, 2])
    if hwe:
        stats["hwe_p"] = rcpp_api.hwe_exact(c, device=device)
    return stats


def FilterMarkers(geno, maf=None, max_missing=None, drop_monomorphic=False, bed=None, stats=None, outdir=None, availmemGb=8,
                  message=None, device=0, hwe=None):
    """A panel without the markers a QC filter drops -> geno dict {asciifileM, asciifileMt, dim_of_ascii_M, marker_index}:
    marker_index = int64, the kept markers' 0-based indices in the panel `geno` came from (composed with geno's own marker_index
    when it is itself a filtered panel).  The rules are marker_keep_mask's on `stats` (default MarkerStats(geno, bed); with hwe= the
    exact-test p-values are added to statistics that do not hold them).  The files
    are written by rcpp_api.filter_markers into `outdir` (default: a qc/ directory beside the source files; it must not be the
    source's directory) and are what ReadMarker leaves for a genotype file that holds only the kept markers.
    Nothing dropped: the source dict with the identity marker_index, nothing written.  Nothing kept: None, after a message."""
    say = message or (lambda s: None)
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    if stats is None:
        stats = MarkerStats(geno, bed=bed, availmemGb=availmemGb, device=device, hwe=hwe is not None)
    if len(stats["n0"]) != L:
        say(" Error: the marker statistics hold %d markers, the panel %d. " % (len(stats["n0"]), L))
        say(" FilterMarkers has terminated with errors")
        return None
    if hwe is not None and "hwe_p" not in stats:
        stats = dict(stats, hwe_p=HWE(stats, device=device))
    idx = np.flatnonzero(marker_keep_mask(stats, maf=maf, max_missing=max_missing, drop_monomorphic=drop_monomorphic, hwe=hwe)).astype(np.int64)
    base = np.asarray(geno["marker_index"], dtype=np.int64) if "marker_index" in geno else np.arange(L, dtype=np.int64)
    if idx.size == L:
        out = dict(geno)
        out["marker_index"] = base
        return out
    if idx.size == 0:
        say(" Error: no marker passes the filter (maf=%s, max_missing=%s, drop_monomorphic=%s%s). "
            % (maf, max_missing, drop_monomorphic, "" if hwe is None else ", hwe=%s" % hwe))
        say(" FilterMarkers has terminated with errors")
        return None
    srcdir = os.path.dirname(os.path.abspath(geno["asciifileM"]))
    outdir = os.path.abspath(outdir) if outdir else os.path.join(srcdir, "qc")
    if outdir == srcdir or outdir == os.path.dirname(os.path.abspath(geno["asciifileMt"])):
        say(" Error: outdir %s holds the source panel; the filtered files need a directory of their own. " % outdir)
        say(" FilterMarkers has terminated with errors")
        return None
    os.makedirs(outdir, exist_ok=True)
    outM, outMt = os.path.join(outdir, "M.ascii"), os.path.join(outdir, "Mt.ascii")
    dims = rcpp_api.filter_markers(geno["asciifileM"], geno["asciifileMt"], (n, L), idx, outM, outMt, availmemGb, device=device)
    say(" %d of %d markers kept. " % (idx.size, L))
    return {"asciifileM": outM, "asciifileMt": outMt, "dim_of_ascii_M": dims, "marker_index": base[idx]}


def HWE(stats_or_counts, device=0):
    """Hardy-Weinberg exact test per marker -> fp64 p (length L), on the device (rcpp_api.hwe_exact: one marker per thread, the order
    of operations of include/eagle_hip.h section 1b''').  stats_or_counts: the dict of MarkerStats / marker_stats_from_counts (its
    n0, n1, n2), or an integer (L, 3) or (L, 4) array of (n_AA, n_AB, n_BB[, unused]) rows."""
    if hasattr(stats_or_counts, "keys"):
        c = np.stack([np.asarray(stats_or_counts[k], dtype=np.int64).ravel() for k in ("n0", "n1", "n2")], axis=1)
    else:
        c = np.asarray(stats_or_counts)
    return rcpp_api.hwe_exact(c, device=device)


def sample_stats_from_counts(n0, n1, n2, n_missing=None, marker_stats=None):
    """Per-individual statistics from integer genotype counts over the markers of a panel, in numpy fp64 (nothing here touches a
    device): n0 / n1 / n2 = the individual's called genotypes coded 0 / 1 / 2, n_missing = its genotypes without a call (default
    none).  het_rate = n1 / (n0 + n1 + n2);  hom_count = n0 + n2;  call_rate = called / (called + n_missing).  With marker_stats (the
    dict of MarkerStats for the same panel) also the method-of-moments inbreeding coefficient F = (O - E) / (L_i - E):  O = hom_count,
    L_i = the individual's called genotypes (L without missing genotypes) and E = sum over the markers with a called genotype of
    1 - 2 p (1 - p) 2m / (2m - 1), p = the marker's allele frequency and m its called genotypes (the number of individuals without
    missing genotypes): the homozygotes expected of an outbred individual.  F = NaN when L_i = E."""
    n0, n1, n2 = (np.asarray(v, dtype=np.int64).ravel() for v in (n0, n1, n2))
    nm = np.zeros_like(n0) if n_missing is None else np.asarray(n_missing, dtype=np.int64).ravel()
    called = n0 + n1 + n2
    with np.errstate(divide="ignore", invalid="ignore"):
        het_rate = np.where(called > 0, n1 / called.astype(np.float64), np.nan)
        call_rate = np.where(called + nm > 0, called / np.maximum(called + nm, 1).astype(np.float64), 0.0)
    out = {"n0": n0, "n1": n1, "n2": n2, "n_missing": nm, "het_rate": het_rate, "hom_count": n0 + n2, "call_rate": call_rate}
    if marker_stats is not None:
        p = np.asarray(marker_stats["freq"], dtype=np.float64)
        m = (np.asarray(marker_stats["n0"], dtype=np.int64) + np.asarray(marker_stats["n1"], dtype=np.int64)
             + np.asarray(marker_stats["n2"], dtype=np.int64)).astype(np.float64)
        ok = m > 0
        two_m = 2.0 * m[ok]
        E = float(np.sum(1.0 - 2.0 * p[ok] * (1.0 - p[ok]) * two_m / (two_m - 1.0)))
        den = called.astype(np.float64) - E
        with np.errstate(divide="ignore", invalid="ignore"):
            out["F"] = np.where(den != 0.0, ((n0 + n2).astype(np.float64) - E) / np.where(den != 0.0, den, 1.0), np.nan)
        out["expected_hom"] = E
    return out


def SampleStats(geno, bed=None, marker_stats=None, availmemGb=8, device=0):
    """Per-individual QC statistics of a panel -> dict of length-n arrays n0, n1, n2, het_rate, hom_count, F (and expected_hom, the E
    of F): sample_stats_from_counts on the device's counts (rcpp_api.sample_counts on geno["asciifileM"]: k_marker_counts on the
    individual-major image) and on marker_stats (default MarkerStats(geno, bed)).  The text files no longer know which genotypes were
    missing, so without `bed` n1 includes them.  bed = the .bed file (or prefix) the panel was ingested from: the counts are then the
    file's own (rcpp_api.bed_sample_counts), and the dict also holds n_missing and call_rate."""
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    if marker_stats is None:
        marker_stats = MarkerStats(geno, bed=bed, availmemGb=availmemGb, device=device)
    if bed is not None:
        c = rcpp_api.bed_sample_counts(bed_fileset(bed)[0], (n, L), availmemGb, device=device)
        return sample_stats_from_counts(c[:, 0], c[:, 1], c[:, 2], c[:, 3], marker_stats=marker_stats)
    c = rcpp_api.sample_counts(geno["asciifileM"], (n, L), availmemGb, device=device)
    out = sample_stats_from_counts(c[:, 0], c[:, 1], c[:, 2], marker_stats=marker_stats)
    del out["n_missing"], out["call_rate"]
    return out


def sample_keep_mask(stats, min_call_rate=None, het_sd=None):
    """Which individuals a filter keeps (boolean, length n) on the output of SampleStats: keep call_rate >= `min_call_rate` (needs
    SampleStats(bed=)); het_sd drops the individuals whose het_rate lies more than that many standard deviations (n - 1 in the
    denominator) from the mean over the individuals, and those without a called genotype.  sample_drop_index turns the mask into
    what ReshapeM / am.reshape_geno take."""
    n = len(stats["n0"])
    keep = np.ones(n, dtype=bool)
    if min_call_rate is not None:
        if "call_rate" not in stats:
            raise ValueError("sample_keep_mask: min_call_rate needs call rates (SampleStats(..., bed=))")
        keep &= np.asarray(stats["call_rate"], dtype=np.float64) >= float(min_call_rate)
    if het_sd is not None:
        h = np.asarray(stats["het_rate"], dtype=np.float64)
        ok = ~np.isnan(h)
        keep &= ok
        if ok.sum() > 1:
            mean, sd = h[ok].mean(), h[ok].std(ddof=1)
            keep &= ~(np.abs(np.where(ok, h, mean) - mean) > float(het_sd) * sd)
    return keep


def sample_drop_index(keep):
    """The individuals a keep mask drops, 1-based and increasing: the indxNA of ReshapeM and am.reshape_geno."""
    return np.flatnonzero(~np.asarray(keep, dtype=bool)).astype(np.int64) + 1


def king_from_counts(ibs0, hethet):
    """KING-robust kinship (Manichaikul et al. 2010) from rcpp_api.sample_ibs' integer matrices -> fp64 (n, n), pure numpy:
    phi_ij = (double)(hethet_ij - 2 ibs0_ij) / (double)(h_i + h_j), h = diag(hethet) = the individuals' heterozygous genotypes;
    NaN where h_i + h_j = 0.  The diagonal and every duplicate pair are 0.5 exactly."""
    a, hh = np.asarray(ibs0, dtype=np.int64), np.asarray(hethet, dtype=np.int64)
    h = np.diagonal(hh)
    num = (hh - 2 * a).astype(np.float64)
    den = (h[:, None] + h[None, :]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0.0, num / np.where(den != 0.0, den, 1.0), np.nan)


def king_from_pair_counts(ibs0, hethet, hetsum):
    """KING-robust kinship over the markers where both individuals are called, from rcpp_api.bed_sample_ibs' (or bed_ibs_host's) integer
    matrices -> fp64 (n, n), pure numpy: phi_ij = (double)(hethet_ij - 2 ibs0_ij) / (double)hetsum_ij, NaN where hetsum_ij = 0.  Two
    copies of one individual are 0.5 exactly, whatever genotypes are missing in either."""
    a, hh, hs = np.asarray(ibs0, dtype=np.int64), np.asarray(hethet, dtype=np.int64), np.asarray(hetsum, dtype=np.int64)
    num, den = (hh - 2 * a).astype(np.float64), hs.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0.0, num / np.where(den != 0.0, den, 1.0), np.nan)


KING_DEGREES = (("duplicate", 0.354), ("first", 0.177), ("second", 0.0884), ("third", 0.0442))


def king_degree(phi):
    """"duplicate" for phi > 0.354, "first" for phi > 0.177, "second" for phi > 0.0884, "third" for phi > 0.0442, else "unrelated"
    (NaN included) -> list of str."""
    out = []
    for v in np.atleast_1d(np.asarray(phi, dtype=np.float64)).ravel().tolist():
        out.append(next((name for name, cut in KING_DEGREES if v > cut), "unrelated"))
    return out


def Relatedness(geno, threshold=0.0884, availmemGb=8, device=0, bed=None, include=None, min_overlap=1):
    """Duplicated and closely related individuals of a panel -> {"kinship": fp64 (n, n) KING-robust phi (king_from_counts),
    "pairs": int64 (k, 2), 0-based, i < j, sorted: the pairs with phi > threshold (a NaN pair is never one), "phi": their phi,
    "degree": king_degree of it, "ibs0", "hethet": the integer matrices}.  The counts come from the device (rcpp_api.sample_ibs: two
    exact Gram products on the fp4 MFMA over all markers of geno["asciifileM"]); missing genotypes count as heterozygotes, so impute
    them first (ImputeBed, ReadMarker(impute=)) or drop low-call-rate individuals (SampleStats(bed=), sample_keep_mask) -- or give
    bed = the .bed file (or prefix) the panel was ingested from: the counts then come from the file itself, every pair over the markers
    where both are called (rcpp_api.bed_sample_ibs, king_from_pair_counts; a pair with fewer than min_overlap such markers is NaN), and
    the dict also carries "ncalled" and "hetsum".  include = the markers of the .bed file that `geno` holds (a bool mask or 0-based
    indices, e.g. FilterMarkers' or LDPrune's keep-list) when geno is a filtered panel; without it the marker counts must agree.
    related_drop chooses whom to drop."""
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    extra = {}
    if bed is None:
        ibs0, hethet = rcpp_api.sample_ibs(geno["asciifileM"], (n, L), availmemGb, device=device)
        phi = king_from_counts(ibs0, hethet)
    else:
        src_bed, src_bim, _ = bed_fileset(bed)
        Lbed = _count_lines(src_bim) if os.path.isfile(src_bim) else (os.path.getsize(src_bed) - 3) // ((n + 3) // 4)
        if include is None and Lbed != L:
            raise ValueError("Relatedness: %s holds %d markers, the panel %d: give include=, the panel's markers in the .bed file" % (src_bed, Lbed, L))
        inc = _bed_include_mask(include, Lbed, "Relatedness")
        if inc is not None and int(inc.sum()) != L:
            raise ValueError("Relatedness: include names %d markers, the panel holds %d" % (int(inc.sum()), L))
        ncalled, ibs0, hethet, hetsum, _ = rcpp_api.bed_sample_ibs(src_bed, (n, Lbed), inc, int(min_overlap), availmemGb, device=device)
        phi = king_from_pair_counts(ibs0, hethet, hetsum)
        phi[ncalled < int(min_overlap)] = np.nan
        extra = {"ncalled": ncalled, "hetsum": hetsum}
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero(np.triu(phi > float(threshold), k=1))
    pairs = np.stack([i, j], axis=1).astype(np.int64).reshape(-1, 2)
    out = {"kinship": phi, "pairs": pairs, "phi": phi[i, j], "degree": king_degree(phi[i, j]), "ibs0": ibs0, "hethet": hethet}
    out.update(extra)
    return out


def related_drop(pairs, n, priority=None):
    """Whom to drop so that no pair of `pairs` (int (k, 2), 0-based, as Relatedness returns them) remains -> the dropped individuals,
    1-BASED and increasing: the indxNA of ReshapeM / am.reshape_geno (by file or VIEW).  Greedy: drop the individual in the most
    remaining pairs, until none remains; ties go to the lower `priority` (length n, e.g. call rates; NaN lowest) when one is given,
    then to the higher index.  Pure numpy."""
    pr = np.atleast_2d(np.asarray(pairs, dtype=np.int64)).reshape(-1, 2)
    n = int(n)
    if pr.size and (pr.min() < 0 or pr.max() >= n or np.any(pr[:, 0] == pr[:, 1])):
        raise ValueError("related_drop: pairs must name two different individuals in [0, n)")
    prio = None
    if priority is not None:
        prio = np.asarray(priority, dtype=np.float64).ravel()
        if prio.size != n:
            raise ValueError("related_drop: priority holds %d individuals, n = %d" % (prio.size, n))
        prio = np.where(np.isnan(prio), -np.inf, prio)
    adj = [set() for _ in range(n)]
    for i, j in pr.tolist():
        adj[i].add(j)
        adj[j].add(i)
    deg = np.array([len(a) for a in adj], dtype=np.int64)
    dropped = []
    while deg.max(initial=0) > 0:
        cand = np.flatnonzero(deg == deg.max())
        if prio is not None:
            cand = cand[prio[cand] == prio[cand].min()]
        d = int(cand.max())
        for j in adj[d]:
            adj[j].discard(d)
            deg[j] -= 1
        adj[d].clear()
        deg[d] = 0
        dropped.append(d)
    return np.sort(np.asarray(dropped, dtype=np.int64)) + 1


# ---- LD scores and the LD decay curve (include/eagle_hip.h section 1b'''v): the restatement in numpy and the interface ----
LD_STATS_MAX_BINS = 512
LD_SCALE = 1073741824.0      # 2^30: u = (uint64)(r2 * LD_SCALE)


def ld_stats_host(band, chrom=None, pos=None, max_dist=0, edges=None):
    """rcpp_api.ld_stats / bed_ld_stats restated in numpy on any r2 band (ld_band_host(Mt8, window) for the ingested panel,
    bed_ld_host(...)[6] for the .bed file): band = fp64 (L, window), band[i, o - 1] = r2 between markers i and i + o, -1.0 without a pair
    -> (U uint64 (L), cnt int32 (L)), with edges also (bin_sum uint64 (B), bin_pairs int64 (B)).  A pair (i, j = i + o) is eligible iff
    r2 >= 0, chrom[i] == chrom[j] (chrom given) and |pos[j] - pos[i]| <= max_dist (pos given, max_dist > 0); u = (uint64)(r2 * 2^30)
    goes to U_i and U_j, 1 to cnt_i and cnt_j, and u and 1 to the bin b with edges[b] <= d < edges[b + 1], d = |pos[j] - pos[i]| with
    pos and o without.  Integer sums: no order of summation changes a bit."""
    band = np.asarray(band, dtype=np.float64)
    L, window = band.shape
    max_dist = int(max_dist)
    ch = None if chrom is None else np.asarray(chrom).ravel()
    ps = None if pos is None else np.asarray(pos).ravel().astype(np.int64)
    if (ch is not None and ch.size != L) or (ps is not None and ps.size != L):
        raise ValueError("ld_stats_host: chrom and pos hold one entry per marker of the band (%d)" % L)
    if max_dist > 0 and ps is None:
        raise ValueError("ld_stats_host: max_dist needs pos")
    if not 1 <= window <= 256 or L * window > 1 << 33:
        raise ValueError("ld_stats_host: 1 <= window <= 256 and markers x window <= 2^33")
    ed = None
    if edges is not None:
        ed = np.asarray(edges).ravel().astype(np.int64)
        if not 2 <= ed.size <= LD_STATS_MAX_BINS + 1 or np.any(np.diff(ed) <= 0):
            raise ValueError("ld_stats_host: edges must be 2 to %d strictly increasing whole numbers" % (LD_STATS_MAX_BINS + 1))
    U, cnt = np.zeros(L, dtype=np.uint64), np.zeros(L, dtype=np.int64)
    nb = 0 if ed is None else ed.size - 1
    bsum, bpairs = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.int64)
    for o in range(1, min(window, L - 1) + 1):
        r2 = band[:-o, o - 1]
        ok = r2 >= 0.0
        if ch is not None:
            ok &= ch[:-o] == ch[o:]
        d = np.full(L - o, o, dtype=np.int64)
        if ps is not None:
            d = np.abs(ps[o:] - ps[:-o])
            if max_dist > 0:
                ok &= d <= max_dist
        u = np.where(ok, r2 * LD_SCALE, 0.0).astype(np.uint64)              # an exact product, a truncating conversion
        U[:-o] += u
        U[o:] += u
        cnt[:-o] += ok
        cnt[o:] += ok
        if nb:
            b = np.searchsorted(ed, d, side="right") - 1                        # edges[b] <= d < edges[b + 1]
            inb = ok & (b >= 0) & (b < nb)
            np.add.at(bsum, b[inb], u[inb])
            np.add.at(bpairs, b[inb], 1)
    out = (U, cnt.astype(np.int32))
    return out + (bsum, bpairs) if nb else out


def ld_half_decay(edges, pairs, mean_r2):
    """The distance at which LD has halved, off a decay curve: the lower edge of the first non-empty bin whose mean r2 is at most half
    the mean of the first non-empty bin, or None when no bin is (or every bin is empty).  Host numpy."""
    ed, pr, mr = np.asarray(edges).ravel(), np.asarray(pairs).ravel(), np.asarray(mean_r2, dtype=np.float64).ravel()
    if ed.size != pr.size + 1 or mr.size != pr.size:
        raise ValueError("ld_half_decay: B + 1 edges for B bins")
    full = np.flatnonzero(pr > 0)
    if not full.size:
        return None
    hit = full[mr[full] <= 0.5 * mr[full[0]]]              # the first non-empty bin itself only when its mean is 0: no LD to halve
    return ed[hit[0]].item() if hit.size else None


def _ld_stats_source(who, geno, map, bed, include):
    """What LDScore and LDDecay share: (n, L, chrom int32 or None, pos int64 or None, bed file or None, (n, Lbed), include mask or None)."""
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    errs = []
    map = _ld_map(who, map, geno, L, errs.append)
    if map is False:
        raise ValueError(who + ":" + errs[0])
    chrom = pos = None
    if map is not None:
        chrom = np.unique(np.asarray([str(c) for c in map["Chr"]]), return_inverse=True)[1].astype(np.int32)
        pos = np.asarray(map["Pos"]).ravel()
        if not np.array_equal(pos.astype(np.int64), pos):
            raise ValueError("%s: the map's positions must be whole numbers of base pairs" % who)
        pos = pos.astype(np.int64)
    if bed is None:
        if include is not None:
            raise ValueError("%s: include= needs bed=" % who)
        return n, L, chrom, pos, None, None, None
    src_bed, src_bim, src_fam = bed_fileset(bed)
    for f in (src_bed, src_bim, src_fam):
        if not os.path.isfile(f):
            raise ValueError("%s: the file %s could not be found" % (who, f))
    nfam, Lbed = _count_lines(src_fam), _count_lines(src_bim)
    if nfam != n:
        raise ValueError("%s: %s names %d individuals, the panel holds %d" % (who, src_fam, nfam, n))
    if include is None and "marker_index" in geno:
        include = np.asarray(geno["marker_index"], dtype=np.int64).ravel()
    inc = _bed_include_mask(include, Lbed, who)
    if (Lbed if inc is None else int(inc.sum())) != L:
        raise ValueError("%s: include selects %d markers of %s, the panel holds %d" % (who, Lbed if inc is None else int(inc.sum()), src_bed, L))
    return n, L, chrom, pos, src_bed, (n, Lbed), inc


def _ld_stats_call(src, window, max_dist, edges, min_overlap, availmemGb, device, geno):
    n, L, chrom, pos, src_bed, bdims, inc = src
    if src_bed is None:
        return rcpp_api.ld_stats(geno["asciifileMt"], (n, L), int(window), chrom, pos, max_dist, edges, availmemGb, device=device)
    return rcpp_api.bed_ld_stats(src_bed, bdims, int(window), inc, int(min_overlap), chrom, pos, max_dist, edges, availmemGb, device=device)


def LDScore(geno, window=50, map=None, kb=None, bed=None, include=None, min_overlap=1, availmemGb=8, device=0):
    """The LD score of every marker of a panel -> {"score": fp64 (L) = 1.0 + u * 2^-30, "partners": int32 (L), the markers summed over,
    "u": uint64 (L), the exact integer sum}: l_i = 1 + the sum of r2_ij over the markers j at most `window` <= 256 markers from i
    (include/eagle_hip.h section 1b'''v; rcpp_api.ld_stats, the r2 of LDPrune and ImputeBed).  It shows how unevenly the panel tags
    the genome, and is the weight GRM(..., ld_score=) and PCA(..., ld_score=) divide by.  map (ReadBim's dict, as LDPrune takes it):
    markers on other chromosomes are left out, and with kb= those more than kb kilobases away (kb needs a map).  bed = the .bed file
    (or prefix) the panel was ingested from: r2 counted over the individuals called at both markers, at least min_overlap of them
    (rcpp_api.bed_ld_stats, section 1b'''iv); include = the panel's markers in the file, default geno's marker_index.  A monomorphic
    marker has score 1.0."""
    src = _ld_stats_source("LDScore", geno, map, bed, include)
    if kb is not None and src[3] is None:
        raise ValueError("LDScore: kb= needs a map with Chr and Pos entries")
    max_dist = 0 if kb is None else int(round(float(kb) * 1000.0))
    if kb is not None and max_dist < 1:
        raise ValueError("LDScore: kb must be at least 0.001")
    U, cnt = _ld_stats_call(src, window, max_dist, None, min_overlap, availmemGb, device, geno)
    return {"score": 1.0 + U.astype(np.float64) * (1.0 / LD_SCALE), "partners": cnt, "u": U}


def LDDecay(geno, window=256, map=None, bins=None, kb=None, bed=None, include=None, min_overlap=1, availmemGb=8, device=0):
    """The LD decay curve of a panel -> {"edges": int64 (B + 1), "pairs": int64 (B), "mean_r2": fp64 (B), NaN for an empty bin,
    "half_decay": ld_half_decay's distance or None, "sum": uint64 (B), the exact integer sums}: the mean r2 of the pairs of markers at
    most `window` <= 256 markers apart per distance bin (include/eagle_hip.h section 1b'''v) -- what window=, kb= and r2= of LDPrune,
    ImputeBed and tag_markers are read off.  Without a map the distance is the marker offset and the default bins are one per offset,
    edges 1 .. window + 1.  With a map (ReadBim's dict) pairs on different chromosomes do not count, the distance is in base pairs, kb=
    is required (pairs further apart do not count) and the default bins are 50 equal ones up to kb.  bins = the edges themselves (2 to
    513 increasing whole numbers, in markers or base pairs).  bed, include, min_overlap as in LDScore."""
    src = _ld_stats_source("LDDecay", geno, map, bed, include)
    max_dist = 0
    if src[3] is None:
        if kb is not None:
            raise ValueError("LDDecay: kb= needs a map with Chr and Pos entries")
        edges = np.arange(1, int(window) + 2, dtype=np.int64) if bins is None else bins
    else:
        if kb is None:
            raise ValueError("LDDecay: a map needs kb=, the largest distance of a pair in kilobases")
        max_dist = int(round(float(kb) * 1000.0))
        if max_dist < 1:
            raise ValueError("LDDecay: kb must be at least 0.001")
        edges = np.unique(np.rint(np.linspace(0.0, float(max_dist) + 1.0, 51)).astype(np.int64)) if bins is None else bins
    edges = np.asarray(edges).ravel()
    _, _, bsum, pairs = _ld_stats_call(src, window, max_dist, edges, min_overlap, availmemGb, device, geno)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(pairs > 0, bsum.astype(np.float64) / pairs.astype(np.float64) * (1.0 / LD_SCALE), np.nan)
    edges = edges.astype(np.int64)
    return {"edges": edges, "pairs": pairs, "mean_r2": mean, "half_decay": ld_half_decay(edges, pairs, mean), "sum": bsum}


# ---- runs of homozygosity (include/eagle_hip.h section 1b'''vi): the restatement in numpy and the interface ----
def roh_classes_mt8(Mt8):
    """The classes of rule 1 from the int8 marker-major image (L, n), values -1 / 0 / +1 -> uint8 (L, n): 0 hom, 1 het (never 2)."""
    return (np.asarray(Mt8) == 0).astype(np.uint8)


def roh_classes_bed(codes):
    """The classes of rule 1 from the 2-bit codes of a .bed file (read_bed_codes: 0 hom A1, 1 missing, 2 het, 3 hom A2) -> uint8:
    0 hom, 1 het, 2 miss."""
    return np.array([0, 2, 1, 0], dtype=np.uint8)[np.asarray(codes, dtype=np.uint8)]


def roh_host(classes, chrom=None, pos=None, **params):
    """rcpp_api.roh / bed_roh restated in numpy: classes = uint8 (L, n) with 0 hom, 1 het, 2 miss (roh_classes_mt8, roh_classes_bed) ->
    (ind int64 (n, 4), seg int32 (S, 6)), rules 2 to 7 of include/eagle_hip.h section 1b'''vi with the parameters of rcpp_api.roh_params.
    Window counts are differences of cumulative sums along every block; runs are read off the flags' edges.  Integers throughout."""
    cl = np.asarray(classes)
    if cl.ndim != 2 or cl.shape[0] < 1 or cl.shape[1] < 1 or cl.min() < 0 or cl.max() > 2:
        raise ValueError("roh_host: classes must be (L, n) with values 0, 1, 2")
    L, n = cl.shape
    p = rcpp_api.roh_params("roh_host", **params)
    ch = None if chrom is None else np.asarray(chrom).ravel()
    ps = np.arange(L, dtype=np.int64) if pos is None else np.asarray(pos).ravel().astype(np.int64)
    if (ch is not None and ch.size != L) or ps.size != L:
        raise ValueError("roh_host: chrom and pos hold one entry per marker (%d)" % L)
    blk = rcpp_api.roh_blocks(ch, L)
    nb = blk.size - 1
    down = np.diff(ps) < 0
    down[blk[1:-1] - 1] = False
    if down.any():
        raise ValueError("roh_host: pos decreases inside a block (panel marker %d)" % (int(np.flatnonzero(down)[0]) + 1))
    w = p["w"]
    het, miss = cl == 1, cl == 2
    flagged = np.zeros((L, n), dtype=bool)
    for a, e in zip(blk[:-1], blk[1:]):
        lb = int(e - a)
        if lb < w:
            continue
        zero = np.zeros((1, n), dtype=np.int64)
        chet = np.concatenate((zero, np.cumsum(het[a:e], axis=0, dtype=np.int64)))
        cmis = np.concatenate((zero, np.cumsum(miss[a:e], axis=0, dtype=np.int64)))
        homw = ((chet[w:] - chet[:-w]) <= p["win_het"]) & ((cmis[w:] - cmis[:-w]) <= p["win_miss"])      # by window start, lb - w + 1 rows
        cw = np.concatenate((zero, np.cumsum(homw, axis=0, dtype=np.int64)))
        j = np.arange(lb)
        s_lo, s_hi = np.maximum(0, j - w + 1), np.minimum(j, lb - w)
        cover = s_hi - s_lo + 1
        hom = cw[s_hi + 1] - cw[s_lo]
        flagged[a:e] = (hom >= 1) & (hom * 65536 >= p["thr16"] * cover[:, None])
    brk = np.zeros(L + 1, dtype=bool)                      # brk[m]: a run cannot continue from marker m - 1 to m
    brk[blk] = True
    if p["max_gap"] > 0 and L > 1:
        brk[1:L] |= np.diff(ps) > p["max_gap"]
    prev = np.concatenate((np.zeros((1, n), dtype=bool), flagged[:-1]))
    nxt = np.concatenate((flagged[1:], np.zeros((1, n), dtype=bool)))
    first = flagged & (brk[:L, None] | ~prev)
    last = flagged & (brk[1:, None] | ~nxt)
    ii, s = np.nonzero(first.T)                             # sorted by (individual, s); the k-th start pairs with the k-th end
    _, e = np.nonzero(last.T)
    zero = np.zeros((1, n), dtype=np.int64)
    chet = np.concatenate((zero, np.cumsum(het, axis=0, dtype=np.int64)))
    cmis = np.concatenate((zero, np.cumsum(miss, axis=0, dtype=np.int64)))
    nsnp, length = e - s + 1, ps[e] - ps[s]
    nhet, nmiss = chet[e + 1, ii] - chet[s, ii], cmis[e + 1, ii] - cmis[s, ii]
    ok = (nsnp >= p["min_snp"]) & (length >= p["min_len"])
    if p["max_density"] > 0:
        ok &= length <= p["max_density"] * nsnp
    if p["max_het"] >= 0:
        ok &= nhet <= p["max_het"]
    ii, s, e, nsnp, length, nhet, nmiss = (x[ok] for x in (ii, s, e, nsnp, length, nhet, nmiss))
    seg = np.stack([ii, s, e, nhet, nmiss, np.searchsorted(blk, s, side="right") - 1], axis=1).astype(np.int32).reshape(-1, 6)
    ind = np.zeros((n, 4), dtype=np.int64)
    np.add.at(ind[:, 0], ii, 1)
    np.add.at(ind[:, 1], ii, nsnp)
    np.add.at(ind[:, 2], ii, length)
    np.maximum.at(ind[:, 3], ii, length)
    return ind, seg


def roh_incidence(seg, L):
    """The ROH incidence of every marker -> int64 (L): the number of individuals with the marker inside one of their segments (rows of
    rcpp_api.roh's table; an individual's segments do not overlap), by a difference array.  Peaks are the "ROH islands"."""
    seg = np.asarray(seg, dtype=np.int64).reshape(-1, 6)
    L = int(L)
    if seg.size and (seg[:, 1].min() < 0 or seg[:, 2].max() >= L or np.any(seg[:, 2] < seg[:, 1])):
        raise ValueError("roh_incidence: a segment outside [0, %d)" % L)
    d = np.zeros(L + 1, dtype=np.int64)
    np.add.at(d, seg[:, 1], 1)
    np.add.at(d, seg[:, 2] + 1, -1)
    return np.cumsum(d[:L])


def roh_thr16(threshold):
    """thr16 of rule 4 from a fraction in [0, 1]: (int)(threshold * 65536 + 0.5)."""
    t = float(threshold)
    if not 0.0 <= t <= 1.0:
        raise ValueError("ROH: threshold must be in [0, 1]")
    return int(t * 65536.0 + 0.5)


def ROH(geno, map=None, bed=None, include=None, window=50, window_het=1, window_missing=5, threshold=0.05, min_snp=100, min_kb=1000,
        max_density_kb=50, max_gap_kb=1000, max_het=None, availmemGb=8, device=0):
    """Runs of homozygosity of every individual of a panel (include/eagle_hip.h section 1b'''vi; rcpp_api.roh) -> {"segments": the table
    as a dict of arrays (individual, first, last, nsnp, nhet, nmiss, block, pos_first, pos_last, length), "nseg", "total_length",
    "longest": int64 (n), "F_ROH": fp64 (n) = total_length / the sum over the blocks of pos[last] - pos[first] (NaN when that is 0),
    "incidence": int64 (L), roh_incidence's count per marker, "ind", "seg": the integer outputs as returned}.  The rule follows PLINK
    --homozyg as documented -- windows of `window` <= 64 markers with at most window_het heterozygous and window_missing missing calls, a
    marker flagged when at least `threshold` of the windows over it are homozygous, then the segment filters -- and its parameter names;
    agreement with the PLINK program is not claimed.  map (ReadBim's dict, as LDPrune takes it): chromosomes are blocks, lengths are base
    pairs and min_kb, max_density_kb (at most one marker per that many kb), max_gap_kb are converted to base pairs (None: filter off).
    Without a map the position is the marker index and the three kb arguments must be passed as None.  bed = the .bed file (or prefix)
    the panel was ingested from: its missing calls count against window_missing instead of being heterozygotes (rcpp_api.bed_roh);
    include = the panel's markers in the file, default geno's marker_index."""
    src = _ld_stats_source("ROH", geno, map, bed, include)
    n, L, chrom, pos, src_bed, bdims, inc = src
    kb = {"min_kb": min_kb, "max_density_kb": max_density_kb, "max_gap_kb": max_gap_kb}
    if pos is None:
        given = [k for k, v in kb.items() if v is not None]
        if given:
            raise ValueError("ROH: %s needs a map with Chr and Pos entries; without one pass min_kb, max_density_kb and max_gap_kb as None"
                             % ", ".join(given))
    bp = {}
    for k, v in kb.items():
        bp[k] = 0 if v is None else int(round(float(v) * 1000.0))
        if v is not None and bp[k] < 1:
            raise ValueError("ROH: %s must be at least 0.001" % k)
    prm = dict(w=int(window), win_het=int(window_het), win_miss=int(window_missing), thr16=roh_thr16(threshold), min_snp=int(min_snp),
               min_len=bp["min_kb"], max_gap=bp["max_gap_kb"], max_density=bp["max_density_kb"], max_het=-1 if max_het is None else int(max_het))
    if src_bed is None:
        ind, seg = rcpp_api.roh(geno["asciifileMt"], (n, L), chrom, pos, availmemGb, device=device, **prm)
    else:
        ind, seg = rcpp_api.bed_roh(src_bed, bdims, inc, chrom, pos, availmemGb, device=device, **prm)
    return roh_summary(ind, seg, L, chrom, pos)


def roh_summary(ind, seg, L, chrom=None, pos=None):
    """ROH's result from the integer outputs (host arithmetic; F_ROH is the one fp64 division)."""
    ps = np.arange(L, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
    blk = rcpp_api.roh_blocks(chrom, L)
    genome = int(np.sum(ps[blk[1:] - 1] - ps[blk[:-1]]))
    s, e = seg[:, 1].astype(np.int64), seg[:, 2].astype(np.int64)
    table = {"individual": seg[:, 0].copy(), "first": seg[:, 1].copy(), "last": seg[:, 2].copy(), "nsnp": (e - s + 1).astype(np.int32),
             "nhet": seg[:, 3].copy(), "nmiss": seg[:, 4].copy(), "block": seg[:, 5].copy(), "pos_first": ps[s], "pos_last": ps[e],
             "length": ps[e] - ps[s]}
    with np.errstate(divide="ignore", invalid="ignore"):
        f = ind[:, 2].astype(np.float64) / np.float64(genome) if genome > 0 else np.full(ind.shape[0], np.nan)
    return {"segments": table, "nseg": ind[:, 0].copy(), "total_length": ind[:, 2].copy(), "longest": ind[:, 3].copy(), "F_ROH": f,
            "incidence": roh_incidence(seg, L), "ind": ind, "seg": seg}


# ---- pairwise IBD-type segments (include/eagle_hip.h section 1b'''vii): the restatement in numpy and the interface ----
def ibd_genotypes_bed(codes):
    """(g int8, called bool), both (L, n), from the 2-bit codes of a .bed file (read_bed_codes: 0 hom A1, 1 missing, 2 het, 3 hom A2):
    g = -1 / 0 / +1 as on the ingested image, 0 where the call is missing."""
    c = np.asarray(codes, dtype=np.uint8)
    return np.array([-1, 0, 0, 1], dtype=np.int8)[c], c != 1


def ibd_all_pairs(n):
    """All pairs 0 <= i < j < n in row-major upper-triangle order -> int32 (n (n - 1) / 2, 2)."""
    i, j = np.triu_indices(int(n), k=1)
    return np.stack([i, j], axis=1).astype(np.int32).reshape(-1, 2)


def ibd_host(g, called=None, pairs=None, chrom=None, pos=None, **params):
    """rcpp_api.ibd / bed_ibd restated in numpy: g = int8 (L, n) with -1 hom A1, 0 het, +1 hom A2 (the marker-major image), called =
    bool (L, n) or None (everything called; ibd_genotypes_bed gives both from .bed codes) -> (pair int64 (P, 4), seg int32 (S, 6)),
    rules 2 to 8 of include/eagle_hip.h section 1b'''vii with the parameters of rcpp_api.ibd_params.  Pure runs are read off the edges
    of the break matrix of a batch of pairs; chains are runs of linked neighbours (both eligible, one break between, no cut).  Integers
    throughout."""
    G = np.asarray(g)
    if G.ndim != 2 or G.shape[0] < 1 or G.shape[1] < 1 or G.min() < -1 or G.max() > 1:
        raise ValueError("ibd_host: g must be (L, n) with values -1, 0, +1")
    G = G.astype(np.int8)
    L, n = G.shape
    Cm = None if called is None else np.asarray(called, dtype=bool)
    if Cm is not None and Cm.shape != G.shape:
        raise ValueError("ibd_host: called must have the shape of g")
    p = rcpp_api.ibd_params("ibd_host", **params)
    pr = rcpp_api.ibd_pairs("ibd_host", pairs, n)
    if pr is None:
        pr = ibd_all_pairs(n)
    ch = None if chrom is None else np.asarray(chrom).ravel()
    ps = np.arange(L, dtype=np.int64) if pos is None else np.asarray(pos).ravel().astype(np.int64)
    if (ch is not None and ch.size != L) or ps.size != L:
        raise ValueError("ibd_host: chrom and pos hold one entry per marker (%d)" % L)
    blk = rcpp_api.roh_blocks(ch, L)
    down = np.diff(ps) < 0
    down[blk[1:-1] - 1] = False
    if down.any():
        raise ValueError("ibd_host: pos decreases inside a block (panel marker %d)" % (int(np.flatnonzero(down)[0]) + 1))
    cut = np.zeros(L + 2, dtype=bool)                      # cut[m]: a piece starts at marker m; L and L + 1 stand for the end
    cut[blk] = True
    cut[L + 1] = True
    if p["max_gap"] > 0 and L > 1:
        cut[1:L] |= np.diff(ps) > p["max_gap"]
    P = pr.shape[0]
    tab = np.zeros((P, 4), dtype=np.int64)
    rows = []
    step = max(1, (1 << 22) // L)
    for k0 in range(0, P, step):
        ii, jj = pr[k0:k0 + step, 0], pr[k0:k0 + step, 1]
        gi, gj = G[:, ii].T, G[:, jj].T                    # (pairs, L)
        brk = (gi * gj == -1) if p["mode"] == 1 else (gi != gj)
        if Cm is not None:
            brk &= Cm[:, ii].T & Cm[:, jj].T
        clean = ~brk
        edge = np.ones((brk.shape[0], 1), dtype=bool)
        first = clean & (cut[None, :L] | np.concatenate((edge, brk[:, :-1]), axis=1))
        last = clean & (cut[None, 1:L + 1] | np.concatenate((brk[:, 1:], edge), axis=1))
        q, rs = np.nonzero(first)                          # sorted by (pair, start); the k-th start pairs with the k-th end
        _, re = np.nonzero(last)
        if q.size == 0:
            continue
        el = (re - rs + 1 >= p["merge_min"]) if p["merge_min"] >= 1 else np.zeros(q.size, dtype=bool)
        link = (q[1:] == q[:-1]) & (rs[1:] == re[:-1] + 2) & ~cut[re[:-1] + 1] & ~cut[re[:-1] + 2] & el[1:] & el[:-1]
        head = np.concatenate(([True], ~link))
        tail = np.concatenate((~link, [True]))
        hq, cs, ce = q[head], rs[head], re[tail]
        runs = np.diff(np.concatenate((np.flatnonzero(head), [q.size])))
        nsnp, length = ce - cs + 1, ps[ce] - ps[cs]
        ok = (nsnp >= p["min_snp"]) & (length >= p["min_len"])
        hq, cs, ce, runs, nsnp, length = (x[ok] for x in (hq, cs, ce, runs, nsnp, length))
        rows.append(np.stack([ii[hq], jj[hq], cs, ce, runs - 1, np.searchsorted(blk, cs, side="right") - 1], axis=1))
        t = tab[k0:k0 + step]
        np.add.at(t[:, 0], hq, 1)
        np.add.at(t[:, 1], hq, nsnp)
        np.add.at(t[:, 2], hq, length)
        np.maximum.at(t[:, 3], hq, length)
    seg = np.concatenate(rows).astype(np.int32).reshape(-1, 6) if rows else np.zeros((0, 6), dtype=np.int32)
    return tab, seg


def ibd_incidence(seg, L):
    """The number of reported segments over every marker -> int64 (L), from the rows of rcpp_api.ibd's table (a pair listed twice counts
    twice), by a difference array.  Peaks are stretches many pairs share: sweeps and low-diversity regions, the pairwise twin of the ROH
    islands."""
    seg = np.asarray(seg, dtype=np.int64).reshape(-1, 6)
    L = int(L)
    if seg.size and (seg[:, 2].min() < 0 or seg[:, 3].max() >= L or np.any(seg[:, 3] < seg[:, 2])):
        raise ValueError("ibd_incidence: a segment outside [0, %d)" % L)
    d = np.zeros(L + 1, dtype=np.int64)
    np.add.at(d, seg[:, 2], 1)
    np.add.at(d, seg[:, 3] + 1, -1)
    return np.cumsum(d[:L])


def ibd_summary(pairs, tab, seg, L, chrom=None, pos=None):
    """IBD's result from the integer outputs (host arithmetic; `shared` is the one fp64 division, over F_ROH's genome length)."""
    ps = np.arange(L, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
    blk = rcpp_api.roh_blocks(chrom, L)
    genome = int(np.sum(ps[blk[1:] - 1] - ps[blk[:-1]]))
    s, e = seg[:, 2].astype(np.int64), seg[:, 3].astype(np.int64)
    table = {"i": seg[:, 0].copy(), "j": seg[:, 1].copy(), "first": seg[:, 2].copy(), "last": seg[:, 3].copy(), "nsnp": (e - s + 1).astype(np.int32),
             "nbreak": seg[:, 4].copy(), "block": seg[:, 5].copy(), "pos_first": ps[s], "pos_last": ps[e], "length": ps[e] - ps[s]}
    with np.errstate(divide="ignore", invalid="ignore"):
        f = tab[:, 2].astype(np.float64) / np.float64(genome) if genome > 0 else np.full(tab.shape[0], np.nan)
    return {"segments": table, "pairs": pairs, "nseg": tab[:, 0].copy(), "total_length": tab[:, 2].copy(), "longest": tab[:, 3].copy(),
            "shared": f, "ibd_incidence": ibd_incidence(seg, L), "pair": tab, "seg": seg}


def IBD(geno, map=None, bed=None, include=None, pairs=None, mode="ibs1", min_snp=200, min_kb=1000, max_gap_kb=1000, merge_min_snp=100,
        availmemGb=8, device=0):
    """Where two individuals of a panel share their genome (include/eagle_hip.h section 1b'''vii; rcpp_api.ibd) -> {"segments": the
    table as a dict of arrays (i, j, first, last, nsnp, nbreak, block, pos_first, pos_last, length), "pairs": int32 (P, 2), "nseg",
    "total_length", "longest": int64 (P), "shared": fp64 (P) = total_length / the genome length F_ROH uses (NaN when that is 0),
    "ibd_incidence": int64 (L), the number of reported segments over each marker, "pair", "seg": the integer outputs as returned}.
    mode "ibs1": runs without opposite homozygotes, where the pair can share one haplotype (IBD1-type); mode "ibs2": runs of equal
    genotypes, where it can share both (IBD2-type) -- the way IBIS and TRUFFLE work on unphased genotypes; agreement with those programs
    is not claimed.  Pure runs of at least merge_min_snp markers are merged across a single break marker (0: no merging); a segment needs
    min_snp markers and min_kb.  These are IBS runs, so they bound IBD from above: short thresholds report chance sharing.  pairs = int
    (P, 2), 0 <= i < j < n (e.g. Relatedness(...)["pairs"]); None = all pairs.  map (ReadBim's dict, as LDPrune takes it): chromosomes
    are blocks, lengths are base pairs, and min_kb, max_gap_kb are converted to base pairs (None: off).  Without a map the position is
    the marker index and both kb arguments must be passed as None.  On the ingested (het-filled) panel a missing call is a het: it can
    never be an opposite homozygote, so missing calls INFLATE mode "ibs1", and it differs from every called homozygote, so they CUT
    mode "ibs2".  bed = the .bed file (or prefix) the panel was ingested from is the route for un-imputed panels: a marker where either
    individual is not called is never a break (rcpp_api.bed_ibd); include = the panel's markers in the file, default geno's
    marker_index."""
    src = _ld_stats_source("IBD", geno, map, bed, include)
    n, L, chrom, pos, src_bed, bdims, inc = src
    kb = {"min_kb": min_kb, "max_gap_kb": max_gap_kb}
    if pos is None:
        given = [k for k, v in kb.items() if v is not None]
        if given:
            raise ValueError("IBD: %s needs a map with Chr and Pos entries; without one pass min_kb and max_gap_kb as None" % ", ".join(given))
    bp = {}
    for k, v in kb.items():
        bp[k] = 0 if v is None else int(round(float(v) * 1000.0))
        if v is not None and bp[k] < 1:
            raise ValueError("IBD: %s must be at least 0.001" % k)
    prm = dict(mode=mode, min_snp=int(min_snp), min_len=bp["min_kb"], max_gap=bp["max_gap_kb"], merge_min=int(merge_min_snp))
    pr = rcpp_api.ibd_pairs("IBD", pairs, n)
    if src_bed is None:
        tab, seg = rcpp_api.ibd(geno["asciifileM"], (n, L), pr, chrom, pos, availmemGb, device=device, **prm)
    else:
        tab, seg = rcpp_api.bed_ibd(src_bed, bdims, inc, pr, chrom, pos, availmemGb, device=device, **prm)
    return ibd_summary(ibd_all_pairs(n) if pr is None else pr, tab, seg, L, chrom, pos)


def ibd_kinship(ibs1, ibs2):
    """A kinship estimate that needs no allele frequencies -> fp64 (P): (shared_1 + shared_2) / 4 from the `shared` fractions of
    IBD(mode="ibs1") and IBD(mode="ibs2") over the same pairs (the dicts IBD returns, or the arrays).  An ibs2 run lies inside an ibs1
    run, so with k2 = shared_2 and k1 = shared_1 - shared_2 this is k1 / 4 + k2 / 2; two copies of one individual give 0.5.  IBS runs
    bound IBD from above, so this bounds the kinship from above: it is as good as the thresholds are strict."""
    a = np.asarray(ibs1["shared"] if isinstance(ibs1, dict) else ibs1, dtype=np.float64)
    b = np.asarray(ibs2["shared"] if isinstance(ibs2, dict) else ibs2, dtype=np.float64)
    if a.shape != b.shape:
        raise ValueError("ibd_kinship: the two results are over different pairs")
    return (a + b) / 4.0


# ---- Mendel errors and parentage assignment (include/eagle_hip.h section 1b'''viii): the restatement in numpy and the interface ----
def ReadFam(path):
    """The pedigree of a PLINK .fam file (family, individual, father, mother, sex, phenotype per line) -> {"FID", "IID", "Father",
    "Mother", "Sex", "Pheno"}: lists of strings, one entry per individual in file order (the order of the .bed file's individuals)."""
    keys = ("FID", "IID", "Father", "Mother", "Sex", "Pheno")
    out = {k: [] for k in keys}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            t = line.split()
            if not t:
                continue
            if len(t) < 6:
                raise ValueError("%s line %d: a .fam line has 6 fields, found %d" % (path, ln, len(t)))
            for k, v in zip(keys, t):
                out[k].append(v)
    return out


def fam_trios(fam):
    """The trios a .fam file records -> int32 (T, 3) of (child, father, mother) as individual indices in file order.  fam = ReadFam's dict
    or a path.  A parent is looked up inside the child's family; one named 0 or not in the file becomes -1, and individuals with no known
    parent are dropped.  ValueError for an individual listed twice, one that is its own parent, or one whose two parents are the same
    individual."""
    fam = ReadFam(fam) if isinstance(fam, (str, os.PathLike)) else fam
    index = {}
    for i, key in enumerate(zip(fam["FID"], fam["IID"])):
        if key in index:
            raise ValueError("fam_trios: individual %s %s is listed twice" % key)
        index[key] = i
    rows = []
    for i, (fid, iid, pa, ma) in enumerate(zip(fam["FID"], fam["IID"], fam["Father"], fam["Mother"])):
        f = -1 if pa == "0" else index.get((fid, pa), -1)
        m = -1 if ma == "0" else index.get((fid, ma), -1)
        if f < 0 and m < 0:
            continue
        if f == i or m == i or f == m:
            raise ValueError("fam_trios: individual %s %s is its own parent or has one individual as both parents" % (fid, iid))
        rows.append((i, f, m))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


def _mendel_planes(who, g, called):
    G = np.asarray(g)
    if G.ndim != 2 or G.shape[0] < 1 or G.shape[1] < 1 or G.min() < -1 or G.max() > 1:
        raise ValueError("%s: g must be (L, n) with values -1, 0, +1" % who)
    Cm = np.ones(G.shape, dtype=bool) if called is None else np.asarray(called, dtype=bool)
    if Cm.shape != G.shape:
        raise ValueError("%s: called must have the shape of g" % who)
    return (G == -1) & Cm, (G == 1) & Cm, Cm


def mendel_host(g, called, trios):
    """rcpp_api.mendel / bed_mendel restated in numpy: g = int8 (L, n) with -1 hom A1, 0 het, +1 hom A2, called = bool (L, n) or None
    (everything called; ibd_genotypes_bed gives both from .bed codes), trios = int (T, 3) -> (trio int32 (T, 6), marker int32 (L)),
    rules 3 to 5 of include/eagle_hip.h section 1b'''viii by the plane formula on boolean columns.  tests/mendel_truth.py pins it to
    loops over allele sets."""
    A, B, Cm = _mendel_planes("mendel_host", g, called)
    L, n = A.shape
    tr = rcpp_api.mendel_trios("mendel_host", trios, n)
    out = np.zeros((tr.shape[0], 6), dtype=np.int32)
    marker = np.zeros(L, dtype=np.int64)
    none = np.zeros(L, dtype=bool)
    for k, (c, f, m) in enumerate(tr.tolist()):
        Ac, Bc, Cc = A[:, c], B[:, c], Cm[:, c]
        Af, Bf, Cf = (A[:, f], B[:, f], Cm[:, f]) if f >= 0 else (none, none, none)
        Am, Bm, Cmo = (A[:, m], B[:, m], Cm[:, m]) if m >= 0 else (none, none, none)
        Hc = Cc & ~Ac & ~Bc
        X = (Ac & Bf) | (Bc & Af)
        E = X | ((Ac | (Hc & Bf)) & Bm) | ((Bc | (Hc & Af)) & Am)
        out[k] = (np.count_nonzero(Cc & Cf), np.count_nonzero(X), np.count_nonzero(Cc & Cmo), np.count_nonzero((Ac & Bm) | (Bc & Am)),
                  np.count_nonzero(Cc & Cf & Cmo), np.count_nonzero(E))
        marker += E
    return out, marker.astype(np.int32)


def parentage_host(g, called, offspring, sires=None, dams=None, min_overlap=1, allow_self=False):
    """rcpp_api.parentage / bed_parentage restated in numpy -> int32 (n_o, 2, 4): rule 6 of include/eagle_hip.h section 1b'''viii.  With
    x, u, v of rule 3 for a (child, sire), the errors of the candidate (s, d) are |x| + |u & ~x & B_d| + |v & ~x & A_d| -- the three
    parts are disjoint -- so all candidates of an offspring are two matrix products of 0 / 1 entries (exact in fp64: every count is
    below 2^31).  The ranking is a lexicographic sort on (e, ordinal)."""
    A, B, Cm = _mendel_planes("parentage_host", g, called)
    L, n = A.shape
    o, s, d, mo, selfing = rcpp_api.parentage_lists("parentage_host", offspring, sires, dams, n, min_overlap, allow_self)
    none, ones = np.zeros((L, 1), dtype=bool), np.ones((L, 1), dtype=bool)
    As, Bs, Cs = (A[:, s], B[:, s], Cm[:, s]) if s.size else (none, none, ones)      # the unknown parent: no genotype; it does not
    Ad, Bd, Cd = (A[:, d], B[:, d], Cm[:, d]) if d.size else (none, none, ones)      # lower the overlap of the other two
    si = s.astype(np.int64) if s.size else np.array([-1], dtype=np.int64)
    di = d.astype(np.int64) if d.size else np.array([-1], dtype=np.int64)
    Adf, Bdf, Cdf = (x.astype(np.float64) for x in (Ad, Bd, Cd))
    best = np.full((o.size, 2, 4), -1, dtype=np.int32)
    for k, c in enumerate(o.tolist()):
        Ac, Bc, Cc = A[:, c:c + 1], B[:, c:c + 1], Cm[:, c:c + 1]
        Hc = Cc & ~Ac & ~Bc
        X = (Ac & Bs) | (Bc & As)
        U = (Ac | (Hc & Bs)) & ~X
        V = (Bc | (Hc & As)) & ~X
        e = X.sum(axis=0)[:, None] + np.rint(U.T.astype(np.float64) @ Bdf + V.T.astype(np.float64) @ Adf).astype(np.int64)
        ov = np.rint((Cc & Cs).T.astype(np.float64) @ Cdf).astype(np.int64)
        ok = (si[:, None] != c) & (di[None, :] != c) & (ov >= mo)
        if not selfing:
            ok &= (si[:, None] != di[None, :]) | (si[:, None] < 0)
        flat = np.flatnonzero(ok.ravel())                   # the ordinals of the admissible candidates, increasing
        order = flat[np.argsort(e.ravel()[flat], kind="stable")][:2]
        for r, q in enumerate(order.tolist()):
            best[k, r] = (si[q // di.size], di[q % di.size], e.ravel()[q], ov.ravel()[q])
    return best


def mendel_summary(trios, tab, marker, n):
    """Mendel's result from the integer outputs: the rates are the only fp64 divisions."""
    tr = np.asarray(trios, dtype=np.int64).reshape(-1, 3)
    tab = np.asarray(tab)
    e = tab[:, 5].astype(np.int64)
    possible = tab[:, 0].astype(np.int64) + tab[:, 2] - tab[:, 4]      # the child and at least one parent are called
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = np.where(possible > 0, e / possible.astype(np.float64), np.nan)
    as_child, as_parent = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    np.add.at(as_child, tr[:, 0], e)
    for col in (1, 2):
        known = tr[:, col] >= 0
        np.add.at(as_parent, tr[known, col], e[known])
    out = {"trios": np.asarray(trios, dtype=np.int32).reshape(-1, 3), "n_cf": tab[:, 0].copy(), "e_cf": tab[:, 1].copy(), "n_cm": tab[:, 2].copy(),
           "e_cm": tab[:, 3].copy(), "n_trio": tab[:, 4].copy(), "errors": tab[:, 5].copy(), "rate": rate, "errors_as_child": as_child,
           "errors_as_parent": as_parent, "trio": tab}
    if marker is not None:
        out["marker_errors"] = marker
        out["marker_rate"] = marker / np.float64(tr.shape[0])
    return out


def Mendel(geno, trios=None, fam=None, bed=None, include=None, map=None, availmemGb=8, device=0):
    """Is the recorded pedigree right?  The Mendel errors of every trio of a pedigreed panel (include/eagle_hip.h section 1b'''viii;
    rcpp_api.mendel; what PLINK reports as --mendel, agreement with that program is not claimed; every marker is taken as autosomal)
    -> {"trios": int32 (T, 3) of (child, father, mother), -1 = unknown, "n_cf", "e_cf", "n_cm", "e_cm", "n_trio", "errors": int32 (T)
    (markers called in child and father, their opposite homozygotes, the same for the mother, markers called in all three, Mendel
    errors), "rate": fp64 (T) = errors / the markers where the child and at least one parent are called (NaN when there is none),
    "errors_as_child", "errors_as_parent": int64 (n), the errors of the trios an individual is in, "marker_errors": int32 (L), the
    trios with an error at each marker, "marker_rate" = marker_errors / T, "trio": the table as returned; with a map also "SNP"}.
    trios = int (T, 3), or fam = a .fam file (or ReadFam's dict) whose recorded trios are used (fam_trios; default: the .fam of bed).
    On the ingested (het-filled) panel a missing call is a het, which both hides errors (a het parent passes either allele) and makes
    them (a het child of two equal homozygotes); bed = the .bed file (or prefix) the panel was ingested from is the route for
    un-imputed panels: a child that is not called has no error and a parent that is not called can pass either allele
    (rcpp_api.bed_mendel); include = the panel's markers in the file, default geno's marker_index.  mendel_keep_mask turns
    marker_errors into a marker filter."""
    n, L, _, _, src_bed, bdims, inc = _ld_stats_source("Mendel", geno, map, bed, include)
    if trios is None:
        if fam is None and src_bed is None:
            raise ValueError("Mendel: give trios=, fam= or bed=")
        fam = bed_fileset(src_bed)[2] if fam is None else fam
        famd = ReadFam(fam) if isinstance(fam, (str, os.PathLike)) else fam
        if len(famd["IID"]) != n:
            raise ValueError("Mendel: the .fam names %d individuals, the panel holds %d" % (len(famd["IID"]), n))
        trios = fam_trios(famd)
        if trios.shape[0] == 0:
            raise ValueError("Mendel: the .fam records no parent")
    tr = rcpp_api.mendel_trios("Mendel", trios, n)
    if src_bed is None:
        tab, marker = rcpp_api.mendel(geno["asciifileM"], (n, L), tr, availmemGb, device=device)
    else:
        tab, marker = rcpp_api.bed_mendel(src_bed, bdims, tr, inc, availmemGb, device=device)
    out = mendel_summary(tr, tab, marker, n)
    if map is not None and "SNP" in map:
        out["SNP"] = list(map["SNP"])
    return out


def mendel_keep_mask(marker_err, ntrios, max_rate=0.1):
    """bool (L): the markers whose share of trios with a Mendel error is at most max_rate (PLINK's --me per-marker threshold), from
    Mendel's marker_errors -- compared as integers: marker_err <= floor(max_rate * ntrios)."""
    e = np.asarray(marker_err)
    ntrios = int(ntrios)
    if ntrios < 1 or not 0.0 <= float(max_rate) <= 1.0:
        raise ValueError("mendel_keep_mask: ntrios must be at least 1 and max_rate in [0, 1]")
    if e.size and (e.min() < 0 or e.max() > ntrios):
        raise ValueError("mendel_keep_mask: a marker with more errors than trios")
    return e <= int(np.floor(float(max_rate) * ntrios))


def parentage_summary(offspring, best, max_rate=0.01):
    """Parentage's result from the rows of rcpp_api.parentage."""
    b = np.asarray(best).reshape(-1, 2, 4)
    has, has2 = b[:, 0, 2] >= 0, b[:, 1, 2] >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = np.where(has & (b[:, 0, 3] > 0), b[:, 0, 2] / b[:, 0, 3].astype(np.float64), np.nan)
    return {"offspring": np.asarray(offspring, dtype=np.int32), "sire": b[:, 0, 0].copy(), "dam": b[:, 0, 1].copy(), "errors": b[:, 0, 2].copy(),
            "overlap": b[:, 0, 3].copy(), "rate": rate, "runner_sire": b[:, 1, 0].copy(), "runner_dam": b[:, 1, 1].copy(),
            "runner_errors": b[:, 1, 2].copy(), "gap": np.where(has2, b[:, 1, 2] - b[:, 0, 2], -1).astype(np.int32),
            "assigned": has & (rate <= float(max_rate)), "best": b}


def Parentage(geno, offspring, sires=None, dams=None, bed=None, include=None, min_overlap=1, allow_self=False, max_rate=0.01, availmemGb=8,
              device=0):
    """Who are the parents?  For every offspring the pair (sire, dam) of the candidate lists with the fewest Mendel errors, by an
    exhaustive search on the device (include/eagle_hip.h section 1b'''viii rule 6; rcpp_api.parentage) -> {"offspring", "sire", "dam":
    int32 individual indices (-1: none, or the unknown parent), "errors", "overlap": int32, "rate": fp64 = errors / overlap,
    "runner_sire", "runner_dam", "runner_errors": the second-best candidate, "gap": runner_errors - errors (-1 without a runner-up; a
    small gap is an ambiguous assignment, e.g. full sibs among the candidates), "assigned": bool, rate <= max_rate, "best": the rows as
    returned}.  offspring, sires, dams = lists of individual indices without duplicates; an individual may be in several lists and is
    never its own parent.  sires or dams None (or empty) assigns one parent alone.  allow_self admits a candidate that is sire and dam
    at once (selfing plants).  THE RANK IS BY ERROR COUNT, NOT BY RATE: with bed = the .bed file (or prefix) the overlap of a candidate
    is the number of markers called in all three, and min_overlap keeps candidates with few called markers from winning by having had
    few chances to err; on the ingested panel every overlap is L.  Ties go to the candidate earlier in the lists.  The errors of the
    true parents are the genotyping errors, so max_rate is set from the chip's error rate; every marker is taken as autosomal."""
    n, L, _, _, src_bed, bdims, inc = _ld_stats_source("Parentage", geno, None, bed, include)
    lists = rcpp_api.parentage_lists("Parentage", offspring, sires, dams, n, min_overlap, allow_self)
    if not 0.0 <= float(max_rate) <= 1.0:
        raise ValueError("Parentage: max_rate must be in [0, 1]")
    if src_bed is None:
        best = rcpp_api.parentage(geno["asciifileM"], (n, L), lists[0], lists[1], lists[2], lists[3], bool(lists[4]), availmemGb, device=device)
    else:
        best = rcpp_api.bed_parentage(src_bed, bdims, lists[0], lists[1], lists[2], inc, lists[3], bool(lists[4]), availmemGb, device=device)
    return parentage_summary(lists[0], best, max_rate)


# ---- GRM and PCA (include/eagle_hip.h section 1b''''): the exact weighted Gram product on the device, fp64 arithmetic on the host ----
GRM_QMAX = 2097151    # 2^21 - 1: the largest weight rcpp_api.weighted_gram takes


def grm_weights(n0, n1, n2, method="standardized", maf=0.0, include=None, ld_score=None):
    """The integer marker weights of a relationship matrix from genotype counts -> (q uint32 (L), scale fp64, used bool (L)), in
    numpy (nothing here touches a device).  Per marker, in int64:  N = n0 + n1 + n2,  c = 2 n2 + n1 (copies of the allele coded 2),
    den = c (2N - c).  A marker is USED iff den > 0 (it is polymorphic), (double)min(c, 2N - c) >= maf * (double)(2N), and `include`
    (bool, length L) is None or true for it.  Unused markers get q = 0.
    "standardized" (EIGENSTRAT / PLINK / GCTA): the weight is w = 1 / (2 p (1 - p)), p = c / (2N), evaluated as
    w = ((2.0 * (double)N) * (double)N) / (double)den;  scale = 2097151.0 / max(w over the used markers);  q = rint(w * scale).
    Every operation is one correctly rounded fp64 operation in that order, so a scalar restatement gives the same bits.
    "vanraden1": q = 1 on the used markers, scale = 1.0 (the weights are exact).
    q / scale stands for w with an absolute error of at most 0.5 / scale, so the RELATIVE error of a marker's weight is at most
    w_max / (w_m (2^22 - 2)), about w_max / (w_m 2^22): 2.4e-6 at worst on a panel with allele frequencies in 0.1 .. 0.9, but a marker
    at p = 0.5 beside one with a single copy of the rare allele among 10,000 individuals loses all but a few bits.  That is why PCA
    defaults to maf = 0.01.  With no used marker q = 0 and scale = 1.0.
    ld_score (default None, and then every bit is as described above): fp64 (L), every entry >= 1 (LDScore(...)["score"]).  Markers in
    LD-dense regions count for less, the LDAK / GCTA-LDMS idea in its simplest form: "standardized" becomes
    w = (((2.0 * (double)N) * (double)N) / (double)den) / ld_score, one more correctly rounded operation, then scale and q as above;
    "vanraden1" becomes w = 1.0 / ld_score with scale = 2097151.0 / max(w over the used markers) and q = rint(w * scale) in the place of
    q = 1 (grm_from_gram then weights its denominator by q / scale as well).  An LD score lies in [1, 1 + 2 * 256], so
    it widens the dynamic range w_max / w_m of the relative error above by a factor of up to 513."""
    n0, n1, n2 = (np.asarray(v, dtype=np.int64).ravel() for v in (n0, n1, n2))
    if method not in ("standardized", "vanraden1"):
        raise ValueError("grm_weights: method must be \"standardized\" or \"vanraden1\"")
    ls = None
    if ld_score is not None:
        ls = np.asarray(ld_score, dtype=np.float64).ravel()
        if ls.size != n0.size or not np.all(ls >= 1.0) or not np.all(np.isfinite(ls)):
            raise ValueError("grm_weights: ld_score must hold one finite number >= 1 per marker (%d)" % n0.size)
    N = n0 + n1 + n2
    c = 2 * n2 + n1
    den = c * (2 * N - c)
    used = (den > 0) & (np.minimum(c, 2 * N - c).astype(np.float64) >= float(maf) * (2 * N).astype(np.float64))
    if include is not None:
        inc = np.asarray(include, dtype=bool).ravel()
        if inc.size != N.size:
            raise ValueError("grm_weights: include holds %d markers, the counts %d" % (inc.size, N.size))
        used &= inc
    q = np.zeros(N.size, dtype=np.uint32)
    if not used.any():
        return q, 1.0, used
    if method == "vanraden1":
        if ls is None:
            q[used] = 1
            return q, 1.0, used
        w = 1.0 / ls[used]
    else:
        Nf = N[used].astype(np.float64)
        w = ((2.0 * Nf) * Nf) / den[used].astype(np.float64)
        if ls is not None:
            w = w / ls[used]
    scale = float(GRM_QMAX) / float(w.max())
    q[used] = np.rint(w * scale).astype(np.uint32)
    return q, scale, used


def _grm_reference(reference, n):
    """The individuals R of a relationship matrix's centring: int64 0-based indices, distinct and increasing; None = everyone."""
    if reference is None:
        return np.arange(n, dtype=np.int64)
    R = np.atleast_1d(np.asarray(reference))
    if R.dtype == bool:
        if R.size != n:
            raise ValueError("reference: a mask of %d individuals, n = %d" % (R.size, n))
        R = np.flatnonzero(R)
    R = np.unique(R.astype(np.int64).ravel())
    if R.size == 0 or R[0] < 0 or R[-1] >= n:
        raise ValueError("reference: individuals must lie in [0, %d) and one at least is needed" % n)
    return R


def _grm_denominator(q_info):
    """D of G = Gc / D (grm_from_gram's docstring), one fp64 number from q_info."""
    used = np.asarray(q_info["used"], dtype=bool).ravel()
    L_used = int(used.sum())
    if q_info["method"] == "standardized":
        return float(q_info["scale"]) * float(L_used)
    if q_info["method"] != "vanraden1":
        raise ValueError("grm_from_gram: unknown method %r" % (q_info["method"],))
    n0, n1, n2 = (np.asarray(q_info[k], dtype=np.int64).ravel()[used] for k in ("n0", "n1", "n2"))
    N = n0 + n1 + n2
    c = 2 * n2 + n1
    Nf = N.astype(np.float64)
    scale = float(q_info.get("scale", 1.0))
    if scale == 1.0:
        return float(np.sum((c * (2 * N - c)).astype(np.float64) / ((2.0 * Nf) * Nf)))
    wq = np.asarray(q_info["q"]).ravel()[used].astype(np.float64) / scale
    return scale * float(np.sum(wq * ((c * (2 * N - c)).astype(np.float64) / ((2.0 * Nf) * Nf))))


def grm_from_gram(Q, q_info, reference=None):
    """The relationship matrix from the integer Gram product Q = rcpp_api.weighted_gram(..., q) -> fp64 (n, n), host numpy.
    q_info = {"method", "scale", "used"} of grm_weights, for "vanraden1" also "n0", "n1", "n2", the counts the weights came from (those
    over R).  R = `reference` (0-based individuals, default all).  With r_i = (1/|R|) sum_{j in R} Q_ij and
    kappa = (1/|R|^2) sum_{i, j in R} Q_ij,
        Gc = Q - r 1^T - 1 r^T + kappa        ( = sum_m q_m (g_im - mu_m)(g_jm - mu_m), mu_m the mean of g_.m over R, because
                                                sum_m q_m mu_m g_im = r_i: centring every marker over R is double-centring Q over R )
        G = Gc / (scale * L_used)             "standardized":  (1 / L_used) sum_m (x_im - 2 p_m)(x_jm - 2 p_m) / (2 p_m (1 - p_m))
        G = Gc / sum_used 2 p_m (1 - p_m)     "vanraden1", 2 p (1 - p) = den / (2 N^2) in grm_weights' terms
    x = g + 1 the allele count, p_m its frequency over R when the counts are R's.  "vanraden1" weights from grm_weights(ld_score=)
    (scale != 1.0; q_info then needs "q" too):  G = Gc / (scale * sum_used (q_m / scale) 2 p_m (1 - p_m)), the same ratio with every
    marker weighted by what stands for 1 / ld_score in Q."""
    Qf = np.asarray(Q).astype(np.float64)       # |Q| < 2^52: exact
    n = Qf.shape[0]
    if Qf.ndim != 2 or Qf.shape[1] != n:
        raise ValueError("grm_from_gram: Q must be square")
    R = _grm_reference(reference, n)
    used = np.asarray(q_info["used"], dtype=bool).ravel()
    L_used = int(used.sum())
    if L_used == 0:
        raise ValueError("grm_from_gram: no marker is used")
    r = Qf[:, R].sum(axis=1) / float(R.size)
    kappa = float(r[R].sum()) / float(R.size)
    Gc = Qf - r[:, None] - r[None, :] + kappa
    return Gc / _grm_denominator(q_info)


def GRM(geno, method="standardized", maf=0.0, include=None, reference=None, stats=None, availmemGb=8, device=0, ld_score=None):
    """The genomic relationship matrix of a panel -> {"G": fp64 (n, n) (grm_from_gram), "Q": int64 (n, n), the exact weighted Gram
    product over ALL n individuals (rcpp_api.weighted_gram: base-128 digit planes of the weights on the int8 MFMA), "q", "scale",
    "used" (grm_weights), "method", "n0", "n1", "n2" (the counts behind the weights), "reference" (int64, 0-based),
    "weight_rel_error": the largest relative error |q / scale - w| / w of a used marker's weight (0 for "vanraden1")}.
    reference = the individuals (0-based indices or a mask) whose allele frequencies centre and scale the markers, default all: the
    counts then come from them alone (MarkerStats on a view of the panel without the others, nothing written), and everyone else is
    placed relative to them -- what PCA(reference=) projects.  stats = a MarkerStats dict of exactly those individuals replaces the
    counting pass.  include = a boolean mask of markers (one chromosome, one MAF bin): the matrix of that subset from the resident
    image, without writing a filtered panel.  ld_score = fp64 (L), LDScore(geno)["score"]: every marker's weight is divided by it
    (grm_weights(ld_score=)), so that LD-dense regions do not dominate the matrix; the dict then carries "ld_score" too."""
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    R = _grm_reference(reference, n)
    if stats is None:
        if R.size == n:
            stats = MarkerStats(geno, availmemGb=availmemGb, device=device)
        else:
            from . import am
            drop = np.setdiff1d(np.arange(n, dtype=np.int64), R) + 1
            stats = MarkerStats(am.reshape_geno(geno, drop, view=True, device=device), availmemGb=availmemGb, device=device)
    n0, n1, n2 = (np.asarray(stats[k], dtype=np.int64).ravel() for k in ("n0", "n1", "n2"))
    if n0.size != L:
        raise ValueError("GRM: the marker statistics hold %d markers, the panel %d" % (n0.size, L))
    q, scale, used = grm_weights(n0, n1, n2, method=method, maf=maf, include=include, ld_score=ld_score)
    if not used.any():
        raise ValueError("GRM: no marker is used (maf=%s%s)" % (maf, "" if include is None else ", include given"))
    Q = rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q, availmemGb, device=device)
    out = {"Q": Q, "q": q, "scale": scale, "used": used, "method": method, "n0": n0, "n1": n1, "n2": n2, "reference": R}
    out["G"] = grm_from_gram(Q, out, reference=R)
    out["weight_rel_error"] = 0.0
    if ld_score is not None:
        out["ld_score"] = np.asarray(ld_score, dtype=np.float64).ravel()
    if method == "standardized" or ld_score is not None:
        if method == "standardized":
            Nf = (n0 + n1 + n2)[used].astype(np.float64)
            w = ((2.0 * Nf) * Nf) / ((2 * n2 + n1) * (2 * (n0 + n1 + n2) - (2 * n2 + n1)))[used].astype(np.float64)
        else:
            w = np.ones(int(used.sum()))
        if ld_score is not None:
            w = w / out["ld_score"][used]
        out["weight_rel_error"] = float(np.max(np.abs(q[used].astype(np.float64) / scale - w) / w))
    return out


def PCA(geno, k=10, method="standardized", maf=0.01, reference=None, grm=None, eig=None, include=None, stats=None, availmemGb=8, device=0,
        ld_score=None, loadings=False):
    """Principal components of the relationship matrix, the covariates of AM(trait, am.add_pcs(X, pca), geno) ->
    {"values": the top k eigenvalues of G[R, R], decreasing, "pcs": fp64 (n, k), "explained": values / trace(G[R, R]), "reference":
    R, "grm": the GRM dict}.  grm = a dict of GRM() (then geno may be None and method / maf / include / stats are not used; its
    reference is R unless `reference` names the same individuals), else GRM(geno, method, maf, include, reference, stats, ld_score=)
    is run (ld_score: LDScore(geno)["score"], the weight of every marker divided by it).
    One eigh of G[R, R]: eig = a callable A -> (values, vectors in columns), in either order of the values (default
    host_model.algebra().eigh: host LAPACK unless host_model.set_algebra("device"); rcpp_api.sym_eig runs it on the device).
    The sign of every vector is fixed so that its component of largest magnitude (the first of equals) is positive.
    Row i of pcs:  for i in R the entries of the unit-norm eigenvectors U;  for i outside R the projection
    (1 / lambda_a) sum_{j in R} G_ij U_ja, which for a member of R is its eigenvector entry exactly (G[R, R] U = U diag(lambda)), so
    a duplicate of a reference individual lands on it.  It is the usual projection and is NOT corrected for shrinkage: with few
    individuals per marker projected individuals sit nearer the origin than reference ones (Lee et al. 2010).
    ValueError for k < 1 or k > |R| - 1 (centring takes one dimension).
    loadings=True (geno is then needed also with grm=): the result also carries the marker loadings that place ANY panel with these
    markers on the components (ProjectPCA), "loadings" fp64 (L, k), "offset" fp64 (k) and "loadings_bound" fp64 (k):
        l_ma = q_m (sum_{j in R} g_jm U_ja) / (D lambda_a),      offset_a = sum_m l_ma mu_m,      mu_m = (n2 - n0) / N over R,
    D the denominator grm_from_gram divides by, so that sum_m l_ma g_im - offset_a is the projection above (no centring term is needed
    inside the sum: sum_{j in R} U_ja = 0 for lambda_a > 0, the constant vector being an eigenvector of the double-centred G[R, R] at
    0).  The inner sums are ONE rcpp_api.marker_scores call: the k eigenvectors, zero outside R, quantised by quantise_weights (scale
    s_a), so every inner sum errs by at most 0.5 |R| / s_a and loadings_bound[a] = max_m q_m 0.5 |R| / (s_a D lambda_a) bounds the error
    of every l_ma.  The default False leaves every result and every call as it was."""
    if grm is None:
        grm = GRM(geno, method=method, maf=maf, include=include, reference=reference, stats=stats, availmemGb=availmemGb, device=device,
                  ld_score=ld_score)
    G = np.asarray(grm["G"], dtype=np.float64)
    n = G.shape[0]
    R = np.asarray(grm["reference"], dtype=np.int64)
    if reference is not None and not np.array_equal(_grm_reference(reference, n), R):
        raise ValueError("PCA: reference differs from the one the relationship matrix was centred on")
    k = int(k)
    if k < 1 or k > R.size - 1:
        raise ValueError("PCA: k = %d components of %d reference individuals (1 <= k <= |R| - 1)" % (k, R.size))
    GR = np.ascontiguousarray(G[np.ix_(R, R)])
    lam, U = (eig or host_model.algebra().eigh)(GR)
    lam, U = np.asarray(lam, dtype=np.float64).ravel(), np.asarray(U, dtype=np.float64)
    top = np.argsort(-lam, kind="stable")[:k]
    lam, U = lam[top], U[:, top]
    big = np.argmax(np.abs(U), axis=0)
    U = U * np.where(U[big, np.arange(k)] < 0, -1.0, 1.0)[None, :]
    pcs = (G[:, R] @ U) / lam[None, :]
    pcs[R] = U
    out = {"values": lam, "pcs": pcs, "explained": lam / float(np.trace(GR)), "reference": R, "grm": grm}
    if loadings:
        if geno is None:
            raise ValueError("PCA: loadings=True needs geno")
        out.update(_pca_loadings(lambda v: rcpp_api.marker_scores(geno["asciifileMt"], geno["dim_of_ascii_M"], v, availmemGb, device=device),
                                 grm, R, lam, U))
    return out


def _pca_loadings(marker_scores, grm, R, lam, U):
    """PCA(loadings=True)'s three entries; marker_scores: int (k, n) -> int64 (L, k), the exact M^T V."""
    n = np.asarray(grm["G"]).shape[0]
    V = np.zeros((n, U.shape[1]))
    V[R] = U
    vq, sc = quantise_weights(V)
    S = np.asarray(marker_scores(np.ascontiguousarray(vq.T))).astype(np.float64)          # |S| < 2^53: exact
    q = np.asarray(grm["q"]).astype(np.float64).ravel()
    D = _grm_denominator(grm)
    load = q[:, None] * (S / sc[None, :]) / (D * lam[None, :])
    n0, n1, n2 = (np.asarray(grm[key], dtype=np.int64).ravel() for key in ("n0", "n1", "n2"))
    N = np.maximum(n0 + n1 + n2, 1).astype(np.float64)
    mu = (n2 - n0).astype(np.float64) / N
    return {"loadings": load, "offset": mu @ load, "loadings_bound": float(q.max()) * 0.5 * float(R.size) / (sc * D * lam)}


def ProjectPCA(pca, geno, availmemGb=8, device=0):
    """The individuals of ANY panel with the markers of the PCA's panel, in the same order, on its components -> fp64 (n_new, k):
    Score(geno, pca["loadings"])["score"] - pca["offset"] with pca = PCA(..., loadings=True).  For the PCA's own panel this reproduces
    pca["pcs"] up to the two quantisation bounds (the loadings', times the markers used, twice: score and offset; and Score's own).
    The scores are exact integer sums, so an individual's coordinates depend on its genotypes alone: a duplicate lands on its original
    bit for bit, in whatever panel and order.  Not corrected for shrinkage (PCA's docstring).  ValueError for a panel of another L."""
    if "loadings" not in pca:
        raise ValueError("ProjectPCA: the PCA carries no loadings (PCA(..., loadings=True))")
    load = np.asarray(pca["loadings"], dtype=np.float64)
    L = int(geno["dim_of_ascii_M"][1])
    if load.shape[0] != L:
        raise ValueError("ProjectPCA: the loadings hold %d markers, the panel %d" % (load.shape[0], L))
    return Score(geno, load, availmemGb=availmemGb, device=device)["score"] - np.asarray(pca["offset"], dtype=np.float64)[None, :]


# ---- line scores (include/eagle_hip.h section 1b''''i): exact integer M w and M^T V on the device, quantising and scaling on the host ----
def line_scores_host(G8, w):
    """The numpy restatement of rcpp_api.sample_scores / marker_scores -> int64 (R, T): G8.astype(int64) @ w.T for an image G8 (R, C)
    in {-1, 0, +1} and integer weights w (C,) or (T, C)."""
    w = np.asarray(w)
    w = w[None, :] if w.ndim == 1 else w
    return np.asarray(G8).astype(np.int64) @ w.astype(np.int64).T


def score_digits_host(w):
    """The four balanced base-256 digit planes of integer weights |w| <= 2^30 -> int8 (4,) + w.shape with
    w = d0 + 256 d1 + 256^2 d2 + 256^3 d3, d in [-128, 127]:  d_p = ((w_p + 128) & 255) - 128,  w_{p+1} = (w_p - d_p) >> 8."""
    x = np.asarray(w).astype(np.int64)
    if x.size and np.abs(x).max() > rcpp_api.SCORES_MAX_WEIGHT:
        raise ValueError("score_digits_host: a weight is beyond +-2^30")
    planes = np.zeros((4,) + x.shape, dtype=np.int8)
    for p in range(4):
        d = ((x + 128) & 255) - 128
        planes[p] = d
        x = (x - d) >> 8
    return planes


def quantise_weights(w, bits=30):
    """Real weights as integers for the exact score pass -> (wq int32, scale), per column of w (C,) or (C, T); scale is a float for
    a vector and fp64 (T,) for a matrix.  scale = 2^e, the largest power of two with max|w| * scale <= 2^bits (so the product is
    exact and rint rounds the true value), wq = rint(w * scale); a zero column gives scale 1.0; a non-finite entry raises ValueError.
    |w - wq / scale| <= 0.5 / scale, so a score over C characters g in {-1, 0, +1} errs by at most 0.5 C / scale < C max|w| 2^-29 at
    the default bits = 30 (scale > 2^29 / max|w|)."""
    wa = np.asarray(w, dtype=np.float64)
    if wa.ndim not in (1, 2) or not 1 <= int(bits) <= 30:
        raise ValueError("quantise_weights: w must be (C,) or (C, T) and 1 <= bits <= 30")
    if not np.all(np.isfinite(wa)):
        raise ValueError("quantise_weights: a weight is not finite")
    cols = wa.reshape(wa.shape[0], -1)
    mx = np.abs(cols).max(axis=0) if cols.shape[0] else np.zeros(cols.shape[1])
    f, x = np.frexp(mx)                                   # mx = f 2^x, 0.5 <= f < 1
    e = np.clip(int(bits) - x + (f == 0.5), -1022, 1023)
    scale = np.where(mx > 0, np.ldexp(1.0, e.astype(np.int64)), 1.0)
    wq = np.rint(cols * scale[None, :]).astype(np.int32)
    return (wq.ravel(), float(scale[0])) if wa.ndim == 1 else (wq, scale)


def Score(geno, weights, include=None, dosage=False, availmemGb=8, device=0):
    """A weighted allele sum per individual, what PLINK --score computes -> {"score": fp64 (n, T) = S / scale, "S": int64 (n, T), the
    exact sums sum_m wq_tm g_im (rcpp_api.sample_scores: balanced base-256 digit planes of the weights on the int8 MFMA), "wq" int32
    (L, T), "scale" fp64 (T,) (quantise_weights), "bound" fp64 (T,)}.  weights: fp64 (L,) or (L, T), one column per score.
    include = a boolean mask of markers: the other markers' weights are zero.  g in {-1, 0, +1} = AA, AB, BB; dosage=True scores the
    0 / 1 / 2 allele count instead, S + sum_m wq_m per column (host arithmetic on wq).
    |score - the fp64 product| <= bound = 0.5 (used markers) / scale, twice that with dosage (an allele count reaches 2), plus the
    rounding of the fp64 product itself."""
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    wa = np.asarray(weights, dtype=np.float64)
    wa = wa.reshape(-1, 1) if wa.ndim == 1 else wa
    if wa.ndim != 2 or wa.shape[0] != L:
        raise ValueError("Score: the weights hold %s entries, the panel %d markers" % (wa.shape[0] if wa.ndim else 0, L))
    used = L
    if include is not None:
        inc = np.asarray(include, dtype=bool).ravel()
        if inc.size != L:
            raise ValueError("Score: include holds %d markers, the panel %d" % (inc.size, L))
        wa = np.where(inc[:, None], wa, 0.0)
        used = int(inc.sum())
    wq, scale = quantise_weights(wa)
    S = rcpp_api.sample_scores(geno["asciifileM"], (n, L), np.ascontiguousarray(wq.T), availmemGb, device=device)
    if dosage:
        S = S + wq.astype(np.int64).sum(axis=0)[None, :]
    return {"score": S.astype(np.float64) / scale[None, :], "S": S, "wq": wq, "scale": scale,
            "bound": (1.0 if dosage else 0.5) * float(used) / scale}


def _ld_sv(stats, n):
    """s = sum g, q = sum g^2 and v = n q - s^2 per marker (int64) from the counts in `stats`, with g = -1 / 0 / +1 for '0' / '1' / '2'."""
    n0, n2 = np.asarray(stats["n0"], dtype=np.int64).ravel(), np.asarray(stats["n2"], dtype=np.int64).ravel()
    s, q = n2 - n0, n2 + n0
    return s, int(n) * q - s * s


def ld_r2_from_dots(dots, stats, loci, n):
    """r^2 between every marker and the markers `loci` (0-based) -> fp64 (L, k), from dots = rcpp_api.ld_dots (int (L, k)), the
    counts n0 / n2 in `stats` (MarkerStats without bed=: the counts of the int8 image) and the n individuals: c = n d - s_i s_j,
    v = n q - s^2 in int64, r^2 = c^2 / (v_i v_j) in fp64.  NaN where either marker is monomorphic.  Pure numpy."""
    d = np.asarray(dots, dtype=np.int64)
    lv = np.atleast_1d(np.asarray(loci, dtype=np.int64)).ravel()
    d = d.reshape(-1, lv.size)
    s, v = _ld_sv(stats, n)
    if s.size != d.shape[0]:
        raise ValueError("ld_r2_from_dots: the statistics hold %d markers, dots %d" % (s.size, d.shape[0]))
    c = (int(n) * d - s[:, None] * s[lv][None, :]).astype(np.float64)
    den = v.astype(np.float64)[:, None] * v[lv].astype(np.float64)[None, :]
    ok = (v[:, None] > 0) & (v[lv][None, :] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, c * c / np.where(ok, den, 1.0), np.nan)


def _ld_pairs(mask, window, rows_per_block=1 << 16):
    """(i, j), i < j: the pairs whose bit is set in an rcpp_api.ld_window mask, in row-major order."""
    m = np.ascontiguousarray(mask, dtype="<u8")
    L = m.shape[0]
    if L == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    m = m.reshape(L, -1)
    if m.shape[1] != (int(window) + 63) // 64:
        raise ValueError("ld_prune_keep: the mask has %d words per marker, window %d needs %d" % (m.shape[1], window, (int(window) + 63) // 64))
    I, J = [], []
    for r0 in range(0, L, rows_per_block):
        bits = np.unpackbits(m[r0:r0 + rows_per_block].view(np.uint8), axis=1, bitorder="little")[:, :int(window)]
        i, o = np.nonzero(bits)
        I.append(i.astype(np.int64) + r0)
        J.append(i.astype(np.int64) + r0 + o + 1)
    I, J = np.concatenate(I), np.concatenate(J)
    ok = J < L
    return I[ok], J[ok]


def ld_prune_keep(mask, window, priority=None, chrom=None, pos=None, kb=None):
    """Greedy LD pruning on the host -> boolean keep vector (length L); pure numpy, no device.  mask = rcpp_api.ld_window's (L, W)
    uint64 words for `window`.  A pair (i, j) counts iff its bit is set, chrom[i] == chrom[j] (when chrom is given) and
    |pos[i] - pos[j]| <= 1000 kb (when pos and kb are given).  The markers are visited in index order, or with `priority` in descending
    priority with ties broken by index (NaN last); a marker is kept unless a marker already kept is paired with it.  A marker in LD with
    nothing -- every monomorphic one, which is FilterMarkers' business -- is always kept."""
    I, J = _ld_pairs(mask, window)
    L = np.asarray(mask).shape[0]
    ok = np.ones(I.size, dtype=bool)
    if chrom is not None:
        ch = np.asarray(chrom)
        if ch.size != L:
            raise ValueError("ld_prune_keep: chrom names %d markers, the mask %d" % (ch.size, L))
        ok &= ch[I] == ch[J]
    if kb is not None:
        if pos is None:
            raise ValueError("ld_prune_keep: kb needs pos")
        ps = np.asarray(pos, dtype=np.float64)
        if ps.size != L:
            raise ValueError("ld_prune_keep: pos holds %d markers, the mask %d" % (ps.size, L))
        ok &= np.abs(ps[I] - ps[J]) <= 1000.0 * float(kb)
    I, J = I[ok], J[ok]
    keep = np.ones(L, dtype=bool)
    if not I.size:
        return keep
    a, b = np.concatenate([I, J]), np.concatenate([J, I])      # both directions, as rows of a CSR adjacency
    srt = np.argsort(a, kind="stable")
    b = b[srt]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=L))])
    if priority is None:
        order = np.flatnonzero(np.diff(ptr) > 0)               # markers without a pair are kept whenever they are visited
    else:
        pr = np.asarray(priority, dtype=np.float64).ravel()
        if pr.size != L:
            raise ValueError("ld_prune_keep: priority holds %d markers, the mask %d" % (pr.size, L))
        order = np.argsort(-np.where(np.isnan(pr), -np.inf, pr), kind="stable")
    blocked = np.zeros(L, dtype=bool)
    for i in order.tolist():
        if blocked[i]:
            keep[i] = False
        else:
            blocked[b[ptr[i]:ptr[i + 1]]] = True
    return keep


def _ld_map(who, map, geno, L, say):
    """The map (ReadBim's dict) of the L markers of `geno`: as given, or the source panel's indexed by geno's marker_index."""
    if map is None:
        return None
    if not hasattr(map, "keys") or "Chr" not in map or "Pos" not in map:
        say(" Error: %s needs a map with Chr and Pos entries (ReadBim's). " % who)
        return False
    if len(map["Chr"]) != L and "marker_index" in geno and len(map["Chr"]) > int(np.max(geno["marker_index"])):
        map = subset_map(map, geno)
    if len(map["Chr"]) != L or len(map["Pos"]) != L:
        say(" Error: the map names %d markers, the panel holds %d. " % (len(map["Chr"]), L))
        return False
    return map


def LDPrune(geno, window=50, r2=0.2, prefer="position", map=None, kb=None, stats=None, outdir=None, availmemGb=8, message=None, device=0,
            bed=None, min_overlap=None):
    """A panel without the markers greedy LD pruning drops -> what FilterMarkers returns: {asciifileM, asciifileMt, dim_of_ascii_M,
    marker_index}, marker_index composed with geno's own.  The pairs in LD come from the device (rcpp_api.ld_window: pairs at most
    `window` <= 256 markers apart with r^2 > `r2`, the exact rule of include/eagle_hip.h section 1b''), the greedy choice is
    ld_prune_keep's on the host, the files are rcpp_api.filter_markers'.  prefer="position" visits the markers in index order (the first
    of a correlated run stays); prefer="maf" visits them by descending minor allele frequency (`stats`, default MarkerStats(geno)).
    map (ReadBim's dict for this panel, or for its source panel when geno carries marker_index): pairs on different chromosomes do
    not count, nor, with kb=, pairs more than kb kilobases apart.  outdir: default an ld/ directory beside the source files; it must
    not be the source's directory.  Nothing dropped: the source dict with the identity marker_index, nothing written.
    bed = the .bed file (or prefix) the panel was ingested from (default None, and then nothing here differs from the lines above): the
    pairs come from the file itself, every pair of markers counted over the individuals called at both, as PLINK --indep-pairwise
    counts them (rcpp_api.bed_ld_window, include/eagle_hip.h section 1b'''iv), so that an un-imputed panel can be pruned before it is
    imputed.  A filtered panel's markers in the file are its marker_index; a pair with fewer than min_overlap both-called individuals
    (default max(2, n // 10)) is not in LD.  The .fam file must name the panel's n individuals."""
    say = message or (lambda s: None)
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])

    def fail(text):
        say(text)
        say(" LDPrune has terminated with errors")
        return None
    if prefer not in ("position", "maf"):
        return fail(' Error: prefer must be "position" or "maf". ')
    errs = []
    map = _ld_map("LDPrune", map, geno, L, errs.append)
    if map is False:
        return fail(errs[0])
    if kb is not None and map is None:
        return fail(" Error: kb= needs a map with Chr and Pos entries. ")
    priority = None
    if prefer == "maf":
        if stats is None:
            stats = MarkerStats(geno, availmemGb=availmemGb, device=device)
        if len(stats["maf"]) != L:
            return fail(" Error: the marker statistics hold %d markers, the panel %d. " % (len(stats["maf"]), L))
        priority = stats["maf"]
    srcdir = os.path.dirname(os.path.abspath(geno["asciifileM"]))
    outdir = os.path.abspath(outdir) if outdir else os.path.join(srcdir, "ld")
    if outdir == srcdir or outdir == os.path.dirname(os.path.abspath(geno["asciifileMt"])):
        return fail(" Error: outdir %s holds the source panel; the pruned files need a directory of their own. " % outdir)
    if bed is None:
        mask, npairs = rcpp_api.ld_window(geno["asciifileMt"], (n, L), window, r2, availmemGb, device=device, return_pairs=True)
    else:
        src_bed, src_bim, src_fam = bed_fileset(bed)
        for f in (src_bed, src_bim, src_fam):
            if not os.path.isfile(f):
                return fail(" Error: the file %s could not be found. " % f)
        nfam, Lbed = _count_lines(src_fam), _count_lines(src_bim)
        if nfam != n:
            return fail(" Error: %s names %d individuals, the panel holds %d. " % (src_fam, nfam, n))
        include = None
        if "marker_index" in geno:
            idx0 = np.asarray(geno["marker_index"], dtype=np.int64).ravel()
            if idx0.size != L or (L and (idx0.min() < 0 or idx0.max() >= Lbed or np.any(np.diff(idx0) <= 0))):
                return fail(" Error: the panel's marker_index does not name %d markers of %s in file order. " % (L, src_bed))
            include = np.zeros(Lbed, dtype=bool)
            include[idx0] = True
        elif Lbed != L:
            return fail(" Error: %s holds %d markers, the panel %d and no marker_index. " % (src_bed, Lbed, L))
        mo = max(2, n // 10) if min_overlap is None else int(min_overlap)
        mask, npairs = rcpp_api.bed_ld_window(src_bed, (n, Lbed), window, r2, include, mo, availmemGb, device=device, return_pairs=True)
    say(" %d pairs of markers within %d markers of each other have r2 above %s. " % (npairs, int(window), r2))
    keep = ld_prune_keep(mask, window, priority=priority, chrom=None if map is None else map["Chr"],
                         pos=None if map is None else map["Pos"], kb=kb)
    idx = np.flatnonzero(keep).astype(np.int64)
    base = np.asarray(geno["marker_index"], dtype=np.int64) if "marker_index" in geno else np.arange(L, dtype=np.int64)
    if idx.size == L:
        out = dict(geno)
        out["marker_index"] = base
        return out
    os.makedirs(outdir, exist_ok=True)
    outM, outMt = os.path.join(outdir, "M.ascii"), os.path.join(outdir, "Mt.ascii")
    dims = rcpp_api.filter_markers(geno["asciifileM"], geno["asciifileMt"], (n, L), idx, outM, outMt, availmemGb, device=device)
    say(" %d of %d markers kept. " % (idx.size, L))
    return {"asciifileM": outM, "asciifileMt": outMt, "dim_of_ascii_M": dims, "marker_index": base[idx]}


def LDofLoci(geno, loci, stats=None, availmemGb=8, device=0):
    """LD of every marker of a panel with the markers `loci` (0-based, any number; repeats allowed) -> {"loci": int64 (k), "dots": int32
    (L, k) = sum over the individuals of g_i g_j, "r2": fp64 (L, k)}.  The dot products run on the device (rcpp_api.ld_dots, 64 loci
    to a pass), r^2 is ld_r2_from_dots on `stats` (default MarkerStats(geno): it must hold the counts of the files, not a .bed's)."""
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    lv = np.atleast_1d(np.asarray(loci, dtype=np.int64)).ravel()
    if stats is None:
        stats = MarkerStats(geno, availmemGb=availmemGb, device=device)
    parts = [rcpp_api.ld_dots(geno["asciifileMt"], (n, L), lv[c0:c0 + 64], availmemGb, device=device) for c0 in range(0, max(lv.size, 1), 64)]
    dots = np.concatenate(parts, axis=1)
    return {"loci": lv, "dots": dots, "r2": ld_r2_from_dots(dots, stats, lv, n)}


def subset_map(map, geno):
    """The marker map of a filtered panel: `map` (ReadBim's dict of SNP / Chr / Pos lists, or a list of names) indexed by
    geno["marker_index"], so that SummaryAM(map=...) and a reader of AM()'s picks name the markers of the source panel.  A geno dict
    without marker_index is an unfiltered panel: the map comes back as it is."""
    if map is None or "marker_index" not in geno:
        return map
    idx = [int(i) for i in geno["marker_index"]]
    if isinstance(map, dict):
        return {k: [v[i] for i in idx] for k, v in map.items()}
    return [map[i] for i in idx]


def SummaryAM(AMobj, trait, X, geno, map=None, xnames=None, availmemGb=8, eig=None, backend=None, message=None, device=0):
    """E/R/summary_am.R:78-221 for the dict am.AM() returns, in the eigenbasis of K (am.SummaryAM): the Wald table of
    [X | the picked markers] and the share of phenotype variance explained as the picks are added one at a time.

    trait, X and geno are what AM() was given, NaN included: the rows AMobj["indxNA"] are dropped from trait and X, and from the
    genotypes by the reshape AM() applied (backend.reshape, or am.reshape_geno writing files for a backend without one).  The
    reference hands SummaryAM the caller's un-reshaped geno and so fails whenever a record is missing; this does not.
    backend (default am.HipBackend(device)) supplies calcMMt, extract_geno and reshape.  eig = (lam, U) of K -- what
    am.SpectralBackend().eig holds after AM() -- replaces the one eigh of K.  map: L marker names (or a mapping with "SNP");
    default M1 .. ML.  xnames: the names of X's columns; default "intercept", "X2", ....  The two tables are printed through
    `message` with summary_am.R's format strings.

    Returns None (and sends summary_am.R:117-121's two messages) when AM() selected nothing, else
    {"pvalue": {"effects", "p_value", "W"}, "size": {"effect_names", "estimate", "p_value"}, "R": {"Marker_name",
    "Prop_var_explained"}} of plain lists.  p_value is 1 - pchisq(W, 1) as the reference computes it (0 once W passes ~75);
    W keeps the evidence of those effects."""
    from . import am
    return am.SummaryAM(AMobj, trait, X, geno, map=map, xnames=xnames, availmemGb=availmemGb, eig=eig, backend=backend, message=message,
                        device=device)


def FPR4AM(trait, X, geno, falseposrate=0.05, numreps=200, seed=101, availmemGb=8, quiet=True, message=None, algebra=None, device=0,
           eig=None, chunk=None):
    """The gamma of AM(..., gamma=) for a wanted false positive rate, from numreps permutations of the trait: am.FPR4AM, under the
    name later releases of the package give it (the reference tree has no such function; DESIGN.md section 4.7d defines it)."""
    from . import am
    return am.FPR4AM(trait, X, geno, falseposrate=falseposrate, numreps=numreps, seed=seed, availmemGb=availmemGb, quiet=quiet,
                     message=message, algebra=algebra, device=device, eig=eig, chunk=chunk)


def MarkerEffects(AMobj, trait, X, geno, availmemGb=8, backend=None, device=0):
    """The fitted model of am.AM() as per-marker effects (am.MarkerEffects, which documents arguments and result)."""
    from . import am
    return am.MarkerEffects(AMobj, trait, X, geno, availmemGb=availmemGb, backend=backend, device=device)


def Predict(effects, geno, X=None, availmemGb=8, device=0):
    """Genetic values of the individuals of any panel with the model's markers from MarkerEffects' result (am.Predict)."""
    from . import am
    return am.Predict(effects, geno, X=X, availmemGb=availmemGb, device=device)


# ---- epistasis (include/eagle_hip.h section 1b''''ii): the additive x additive interaction F test between pairs of markers ----
def quantise_trait(y):
    """A real trait as integers for the exact epistasis scan -> (yq int32, scale): the trait is centred at its mean, multiplied by
    scale = the largest power of two that keeps max|y - mean| * scale <= EPI_YMAX = 10^6, and rounded with np.rint.  The F statistic is
    invariant to a shift and a scale of the trait, so all this costs is the rounding: at most half a unit in 10^6 of the trait's
    largest deviation from its mean (between 0.5e-6 and 1e-6 of it, as scale is a power of two) per record.  A constant trait gives zeros
    and scale 1.0; a non-finite record raises ValueError."""
    ya = np.asarray(y, dtype=np.float64).ravel()
    if not np.all(np.isfinite(ya)):
        raise ValueError("quantise_trait: a trait record is not finite (drop NaN records first: am.reshape_geno(view=True))")
    c = ya - ya.mean() if ya.size else ya
    mx = float(np.abs(c).max()) if c.size else 0.0
    if mx == 0.0:
        return np.zeros(ya.size, dtype=np.int32), 1.0
    e = int(np.floor(np.log2(rcpp_api.EPI_YMAX / mx)))
    while np.ldexp(mx, e + 1) <= rcpp_api.EPI_YMAX:
        e += 1
    while np.ldexp(mx, e) > rcpp_api.EPI_YMAX:
        e -= 1
    scale = float(np.ldexp(1.0, e))
    return np.rint(c * scale).astype(np.int32), scale


def _epi_t53(x):
    """x (a Python int) truncated toward zero to its top 53 bits, as a float (exact)."""
    m = -x if x < 0 else x
    sh = max(0, m.bit_length() - 53)
    v = float((m >> sh) << sh)
    return -v if x < 0 else v


def _epi_max(a):
    a = np.asarray(a)
    if a.dtype == object:
        return None
    return int(np.abs(a.astype(np.int64)).max()) if a.size else 0


def _epi_mul(a, b):
    """a * b exactly: in int64 where the operands' magnitudes prove that nothing wraps, else on Python ints (object arrays)."""
    ma, mb = _epi_max(a), _epi_max(b)
    if ma is not None and mb is not None and ma * mb < 1 << 62:
        return np.asarray(a, dtype=np.int64) * np.asarray(b, dtype=np.int64)
    return np.asarray(a).astype(object) * np.asarray(b).astype(object)


def _epi_add(*terms):
    """The exact sum of the terms, by the same rule."""
    mx = [_epi_max(t) for t in terms]
    if all(m is not None for m in mx) and sum(mx) < 1 << 62:
        out = np.asarray(terms[0], dtype=np.int64)
        for t in terms[1:]:
            out = out + np.asarray(t, dtype=np.int64)
        return out
    out = np.asarray(terms[0]).astype(object)
    for t in terms[1:]:
        out = out + np.asarray(t).astype(object)
    return out


def _epi_sums(n, Y, T, mi, mj, mom):
    """Delta, Sxx, Sxy, Syy of rule 3, exact: int64 arrays where the magnitudes allow it, else object arrays of Python ints (_epi_mul,
    _epi_add).  mi, mj: (s, q, u) of the two markers as int64 arrays that broadcast against the leading shape of mom; mom[..., 5]: the
    five pair sums."""
    M, A_ = _epi_mul, _epi_add
    si, qi, ui = (np.asarray(a, dtype=np.int64) for a in mi)
    sj, qj, uj = (np.asarray(a, dtype=np.int64) for a in mj)
    d, e, f, h, z = (np.asarray(mom[..., c], dtype=np.int64) for c in range(5))
    n, Y, T = np.int64(n), np.int64(Y), np.int64(T)
    neg = lambda a: M(a, np.int64(-1))                                    # noqa: E731
    A00, A01, A02 = A_(M(qi, qj), neg(M(d, d))), A_(M(d, sj), neg(M(si, qj))), A_(M(si, d), neg(M(qi, sj)))
    A11, A12, A22 = A_(M(n, qj), neg(M(sj, sj))), A_(M(si, sj), neg(M(n, d))), A_(M(n, qi), neg(M(si, si)))
    Delta = A_(M(n, A00), M(si, A01), M(sj, A02))
    Amat = ((A00, A01, A02), (A01, A11, A12), (A02, A12, A22))
    mv = lambda v: [A_(*[M(Amat[r][c], v[c]) for c in range(3)]) for r in range(3)]      # noqa: E731
    dot = lambda v, w: A_(*[M(v[r], w[r]) for r in range(3)])                            # noqa: E731
    c, u = (d, e, f), (Y, ui, uj)
    Ac, Au = mv(c), mv(u)
    return (Delta, A_(M(Delta, h), neg(dot(c, Ac))), A_(M(Delta, z), neg(dot(u, Ac))), A_(M(Delta, T), neg(dot(u, Au))))


def _epi_t53_array(x):
    """_epi_t53 of every entry of an int64 or object array -> fp64."""
    x = np.asarray(x)
    if x.dtype == object:
        return np.array([_epi_t53(int(v)) for v in x.ravel()], dtype=np.float64).reshape(x.shape)
    m = np.abs(x.astype(np.int64)).astype(np.uint64)                      # |x| < 2^62 here (_epi_add's rule)
    sh = np.zeros(m.shape, dtype=np.uint64)
    for k in range(53, 64):
        sh += (m >> np.uint64(k)) != 0
    v = ((m >> sh) << sh).astype(np.float64)                              # at most 53 significant bits: exact
    return np.where(x < 0, -v, v)


def _epi_stat(n, Delta, Sxx, Sxy, Syy):
    """Rules 4 and 5 on the arrays of _epi_sums -> fp64 of their shape: every fp64 step one numpy operation, in the header's order."""
    shape = np.shape(Delta)
    D, xx, xy, yy = (np.asarray(a).ravel() for a in (Delta, Sxx, Sxy, Syy))
    ok = (np.asarray(D > 0).astype(bool) & np.asarray(xx > 0).astype(bool)) if n > 4 else np.zeros(D.size, dtype=bool)
    stat = np.full(D.size, np.nan)
    idx = np.flatnonzero(ok)
    if idx.size:
        fx, fxy, fy = _epi_t53_array(xx[idx]), _epi_t53_array(xy[idx]), _epi_t53_array(yy[idx])
        with np.errstate(all="ignore"):
            r2 = (fxy / fx) * (fxy / fy)
            st = (np.float64(n - 4) * r2) / (np.float64(1.0) - r2)
        st[~(r2 < 1.0)] = np.inf
        stat[idx] = st
    return stat.reshape(shape)


def epistasis_host(G, yq, loci=None, chrom=None, gap=0, min_stat=0.0, hit_cap=None):
    """The numpy restatement of rcpp_api.epistasis_loci (loci given) and rcpp_api.epistasis_pairs (loci None) on the genotypes G, int8 (n,
    L) in {-1, 0, +1}, and the integer trait yq: integer matrix products for the sums, Python ints for the 128-bit part, numpy fp64 for the
    six rounded operations.  Returns the same tables: {"stat" (L, k), "mom" (L, k, 5)} or epistasis_pairs' dict (hit_cap None: always with
    the tables)."""
    Gi = np.asarray(G, dtype=np.int64)
    n, L = Gi.shape
    y = np.asarray(yq, dtype=np.int64).ravel()
    if y.size != n:
        raise ValueError("epistasis_host: %d trait records for %d individuals" % (y.size, n))
    G2 = Gi * Gi
    Y, T = int(y.sum()), int((y * y).sum())
    s, q, u = Gi.sum(axis=0), G2.sum(axis=0), y @ Gi
    cols = np.arange(L) if loci is None else np.atleast_1d(np.asarray(loci, dtype=np.int64)).ravel()
    Bj, B2 = Gi[:, cols], G2[:, cols]
    # Every term of the five products is an integer of at most max|y| in absolute value, so every partial sum of the n terms, in any
    # order, stays below n max|y|: under 2^53 the fp64 product (BLAS) is the exact integer, and numpy's int64 loop is not needed.
    if n * max(1, int(np.abs(y).max()) if n else 1) < 1 << 53:
        dot = lambda a, b: np.rint(a.astype(np.float64).T @ b.astype(np.float64)).astype(np.int64)      # noqa: E731
    else:
        dot = lambda a, b: a.T @ b                                                                      # noqa: E731
    mom = np.stack([dot(Gi, Bj), dot(G2, Bj), dot(Gi, B2), dot(G2, B2), dot(Gi * y[:, None], Bj)], axis=-1)
    if loci is not None:
        S = _epi_sums(n, Y, T, (s[:, None], q[:, None], u[:, None]), (s[cols][None, :], q[cols][None, :], u[cols][None, :]), mom)
        return {"stat": _epi_stat(n, *S), "mom": mom}
    ii, jj = np.triu_indices(L, 1)
    keep = np.ones(ii.size, dtype=bool)
    if gap > 0:
        same = np.ones(ii.size, dtype=bool) if chrom is None else np.asarray(chrom).ravel()[ii] == np.asarray(chrom).ravel()[jj]
        keep = ~((jj - ii <= gap) & same)
    ii, jj = ii[keep], jj[keep]
    pm = mom[ii, jj]
    stat = _epi_stat(n, *_epi_sums(n, Y, T, (s[ii], q[ii], u[ii]), (s[jj], q[jj], u[jj]), pm))
    defined = ~np.isnan(stat)
    best = (-1, -1, float("nan"))
    if defined.any():
        top = stat[defined].max()
        k = int(np.flatnonzero(defined & (stat == top))[0])          # triu order is (i, j) order
        best = (int(ii[k]), int(jj[k]), float(top))
    hit = np.flatnonzero(defined & (stat >= min_stat))
    out = {"nhits": int(hit.size), "ntested": int(defined.sum()), "max": best, "hit_ij": None, "hit_stat": None, "hit_mom": None}
    if hit_cap is None or hit.size <= hit_cap:
        out.update(hit_ij=np.stack([ii[hit], jj[hit]], axis=1).astype(np.int32), hit_stat=stat[hit], hit_mom=pm[hit])
    return out


def epistasis_effects(n, Y, T, mi, mj, mom, scale=1.0):
    """b3 and its standard error in the trait's own units from the exact sums -> (b3, se) fp64: b3 = Sxy / Sxx and se^2 = (Sxx Syy -
    Sxy^2) / ((n - 4) Sxx^2) over `scale` (quantise_trait's), NaN where the pair is undefined."""
    D, xx, xy, yy = (np.asarray(a, dtype=object) for a in _epi_sums(n, Y, T, mi, mj, mom))
    shape = D.shape
    b3, se = np.full(D.size, np.nan), np.full(D.size, np.nan)
    for k, (dk, a, b, c) in enumerate(zip(D.ravel(), xx.ravel(), xy.ravel(), yy.ravel())):
        if n > 4 and dk > 0 and a > 0:
            b3[k] = (b / a) / scale
            se[k] = math.sqrt(max(a * c - b * b, 0) / (n - 4)) / a / scale      # int / int: true division of Python ints
    return b3.reshape(shape), se.reshape(shape)


def Epistasis(geno, y, loci=None, map=None, gap=0, min_stat=None, p=1e-8, hit_cap=1 << 20, availmemGb=8, device=0):
    """The additive x additive interaction test y = b0 + b1 g_i + b2 g_j + b3 g_i g_j + e between pairs of markers of a panel (PLINK
    --epistasis for a quantitative trait; include/eagle_hip.h section 1b''''ii): the F(1, n - 4) of b3 = 0 from exact integer sums on the
    device.  y: one record per individual; a real trait goes through quantise_trait (which costs at most half a unit in 10^6 of its
    range), an integer one (|y| <= 10^6) is used as it is.  NaN records raise ValueError: drop them with am.reshape_geno(geno, indxNA,
    view=True) and pass the kept records.  A constant trait raises ValueError.

    loci (0-based, any number, repeats allowed): every marker against each of them -> {"loci", "stat" fp64 (L, k), NaN = undefined, "p" =
    scipy.special.fdtrc(1, n - 4, stat), "b3", "se" (trait units), "mom" int64 (L, k, 5), "scale"}.
    loci None: all pairs i < j, except those at most `gap` markers apart on one chromosome (map: ReadBim's dict, its Chr used; None: one
    chromosome) -> {"hits": int32 (H, 2), "stat", "p", "b3", "se", "mom" of the hits sorted by (i, j), "nhits", "ntested": the defined
    pairs, "max": (i, j, stat), "min_stat", "scale"}.  A hit is stat >= min_stat; min_stat None derives it from p: fdtri(1, n - 4, 1 - p).
    With more than hit_cap hits the tables are None and nhits holds the total.  The panel must fit the device (prune or filter first)."""
    from scipy import special
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    ya = np.asarray(y).ravel()
    if ya.size != n:
        raise ValueError("Epistasis: %d trait records for %d genotyped individuals" % (ya.size, n))
    if np.issubdtype(ya.dtype, np.integer):
        yq, scale = ya.astype(np.int64), 1.0
        if yq.size and int(np.abs(yq).max()) > rcpp_api.EPI_YMAX:
            raise ValueError("Epistasis: an integer trait beyond 10^6 in absolute value (pass it as a real trait)")
    else:
        if np.any(np.isnan(ya.astype(np.float64))):
            raise ValueError("Epistasis: the trait holds NaN records; drop them and their genotypes first: am.reshape_geno(geno, indxNA, "
                             "view=True) gives the panel of the kept individuals")
        yq, scale = quantise_trait(ya)
    if yq.size == 0 or int(yq.min()) == int(yq.max()):
        raise ValueError("Epistasis: the trait is constant")
    yq = yq.astype(np.int32)
    Mt, dims = geno["asciifileMt"], (n, L)
    cnt = rcpp_api.marker_counts(Mt, dims, availmemGb, device=device).astype(np.int64)
    s, q = cnt[:, 2] - cnt[:, 0], cnt[:, 2] + cnt[:, 0]
    u = rcpp_api.marker_scores(Mt, dims, yq, availmemGb, device=device)[:, 0]
    Y, T = int(yq.astype(np.int64).sum()), int((yq.astype(np.int64) ** 2).sum())
    pval = lambda st: special.fdtrc(1.0, float(n - 4), st) if n > 4 else np.full(np.shape(st), np.nan)      # noqa: E731
    if loci is not None:
        lv = np.atleast_1d(np.asarray(loci, dtype=np.int64)).ravel()
        parts = [rcpp_api.epistasis_loci(Mt, dims, yq, lv[c0:c0 + 64], availmemGb, device=device) for c0 in range(0, max(lv.size, 1), 64)]
        stat, mom = np.concatenate([a for a, _ in parts], axis=1), np.concatenate([b for _, b in parts], axis=1)
        b3, se = epistasis_effects(n, Y, T, (s[:, None], q[:, None], u[:, None]), (s[lv][None, :], q[lv][None, :], u[lv][None, :]), mom, scale)
        return {"loci": lv, "stat": stat, "p": pval(stat), "b3": b3, "se": se, "mom": mom, "scale": scale}
    chrom = None
    if map is not None:
        m = _ld_map("Epistasis", map, geno, L, lambda text: None)
        if m is False:
            raise ValueError("Epistasis: the map must hold Chr and Pos entries for the panel's %d markers" % L)
        chrom = np.unique(np.asarray(m["Chr"]).astype(str), return_inverse=True)[1].astype(np.int32)
    if min_stat is None:
        if not 0.0 < float(p) < 1.0 or n <= 4:
            raise ValueError("Epistasis: p must lie in (0, 1) and n above 4")
        min_stat = float(special.fdtri(1.0, float(n - 4), 1.0 - float(p)))
    r = rcpp_api.epistasis_pairs(Mt, dims, yq, chrom, int(gap), float(min_stat), int(hit_cap), availmemGb, device=device)
    out = {"hits": r["hit_ij"], "stat": r["hit_stat"], "mom": r["hit_mom"], "p": None, "b3": None, "se": None, "nhits": r["nhits"],
           "ntested": r["ntested"], "max": r["max"], "min_stat": float(min_stat), "scale": scale}
    if r["hit_ij"] is not None:
        i, j = r["hit_ij"][:, 0].astype(np.int64), r["hit_ij"][:, 1].astype(np.int64)
        out["p"] = pval(r["hit_stat"])
        out["b3"], out["se"] = epistasis_effects(n, Y, T, (s[i], q[i], u[i]), (s[j], q[j], u[j]), r["hit_mom"], scale)
    return out


def EpistasisOfLoci(AMobj, trait, X, geno, availmemGb=8, backend=None, device=0):
    """Every marker against the loci AM() reported, on the conditional residual of the fitted model (am.EpistasisOfLoci)."""
    from . import am
    return am.EpistasisOfLoci(AMobj, trait, X, geno, availmemGb=availmemGb, backend=backend, device=device)


# ---- per-group genotype counts, Fst and case/control association (include/eagle_hip.h section 1b''''iii) ----
def group_labels(values):
    """One value per individual (population names, numbers, ...) -> (labels int32 (n), names): labels[i] = the position of values[i] in
    names, the sorted distinct values; None and NaN become -1, in no group."""
    vals = list(np.asarray(values, dtype=object).ravel())
    gone = [v is None or (isinstance(v, (float, np.floating)) and math.isnan(v)) for v in vals]
    kept = {v for v, g in zip(vals, gone) if not g}
    try:
        names = sorted(kept)
    except TypeError:
        names = sorted(kept, key=str)
    where = {v: k for k, v in enumerate(names)}
    return np.array([-1 if g else where[v] for v, g in zip(vals, gone)], dtype=np.int32), names


def _group_onehot(labels, K):
    lv = np.asarray(labels, dtype=np.int64).ravel()
    H = np.zeros((lv.size, int(K)), dtype=np.int64)
    idx = np.flatnonzero(lv >= 0)
    H[idx, lv[idx]] = 1
    return H


def group_counts_host(Mt8, labels, K):
    """rcpp_api.group_counts restated in numpy: Mt8 = int8 (L, n) of -1 / 0 / +1 (marker-major), labels in [-1, K) -> int32 (L, K, 3).
    The device's rule: s = sum of g and q = sum of g^2 over a group, n2 = (q + s) / 2, n0 = (q - s) / 2, n1 = size - q."""
    G = np.asarray(Mt8, dtype=np.int64)
    H = _group_onehot(labels, K)
    s, q, size = G @ H, (G * G) @ H, H.sum(axis=0)[None, :]
    return np.stack([(q - s) // 2, size - q, (q + s) // 2], axis=2).astype(np.int32)


def bed_group_counts_host(codes, labels, K):
    """rcpp_api.bed_group_counts restated in numpy: codes = uint8 (L, n) 2-bit codes (read_bed_codes) -> int32 (L, K, 4) = homozygous
    A1 (code 0), heterozygous (2), homozygous A2 (3), missing (1) per group."""
    c = np.asarray(codes)
    H = _group_onehot(labels, K)
    return np.stack([(c == v).astype(np.int64) @ H for v in (0, 2, 3, 1)], axis=2).astype(np.int32)


def fisher_2x2_host(tables):
    """rcpp_api.fisher_2x2 restated as a scalar fp64 loop in the order of include/eagle_hip.h section 1b''''iii: the same bits."""
    out = []
    for a, b, c, d in np.asarray(tables, dtype=np.int64).reshape(-1, 4).tolist():
        r1, r2, c1 = a + b, c + d, a + c
        N = r1 + r2
        if N == 0:
            out.append(1.0)
            continue
        lo, hi = max(0, c1 - r2), min(r1, c1)
        x0 = min(max((r1 + 1) * (c1 + 1) // (N + 2), lo), hi)

        def walk(cut):
            tail = cut >= 0.0
            total = 1.0 if (not tail or 1.0 <= cut) else 0.0
            pobs = 1.0 if a == x0 else 0.0
            p = 1.0
            for x in range(x0, lo, -1):
                p = (p * float(x * (r2 - c1 + x))) / float((r1 - x + 1) * (c1 - x + 1))
                if p == 0.0:
                    break
                if x - 1 == a:
                    pobs = p
                if not tail or p <= cut:
                    total = total + p
            p = 1.0
            for x in range(x0, hi):
                p = (p * float((r1 - x) * (c1 - x))) / float((x + 1) * (r2 - c1 + x + 1))
                if p == 0.0:
                    break
                if x + 1 == a:
                    pobs = p
                if not tail or p <= cut:
                    total = total + p
            return total, pobs

        total, pobs = walk(-1.0)
        tail, _ = walk(pobs * 1.0000001)
        out.append(min(1.0, tail / total))
    return np.array(out, dtype=np.float64)


def _group_source(who, geno, bed, include):
    """(n, L, bed file or None, (n, Lbed), include mask or None): the checks LDScore makes of a .bed source."""
    n, L, _, _, src_bed, bdims, inc = _ld_stats_source(who, geno, None, bed, include if bed is not None else None)
    return n, L, src_bed, bdims, inc


def GroupCounts(geno, groups, bed=None, include=None, availmemGb=8, device=0):
    """The genotype counts of every marker of a panel within each group of individuals -> {"counts": int32 (L, K, 3) = (n0, n1, n2)
    per marker and group -- with bed= (L, K, 4) = (hom A1, het, hom A2, missing) --, "names": the K group names, "labels": int32 (n),
    "sizes": int64 (K), and "freq", "maf", "het", "call_rate": fp64 (L, K), what marker_stats_from_counts makes of each group's counts}.
    groups: one value per individual (group_labels: None / NaN = in no group).  The counting runs on the device (rcpp_api.group_counts
    on geno["asciifileMt"], one pass over the int8 image on the matrix cores; include/eagle_hip.h section 1b''''iii), the arithmetic on
    the host.  Without `bed` a missing call of the source is a heterozygote, as in MarkerStats; bed = the .bed file (or prefix) the panel
    was ingested from gives the file's own counts (rcpp_api.bed_group_counts), where missing is missing.  include= (a bool mask or marker
    indices; with bed= of the FILE's markers, default geno's marker_index) subsets the rows on the host.  HWE(out["counts"][:, k])
    is the Hardy-Weinberg exact test within group k: with k the controls that is the HWE-in-controls filter."""
    labels, names = group_labels(groups)
    n, L, src_bed, bdims, inc = _group_source("GroupCounts", geno, bed, include)
    if labels.size != n:
        raise ValueError("GroupCounts: %d group entries for %d genotyped individuals" % (labels.size, n))
    K = max(len(names), 1)
    if src_bed is not None:
        c = rcpp_api.bed_group_counts(src_bed, bdims, labels, K, availmemGb, device=device)
    else:
        c = rcpp_api.group_counts(geno["asciifileMt"], (n, L), labels, K, availmemGb, device=device)
        inc = _bed_include_mask(include, L, "GroupCounts")
    if inc is not None:
        c = np.ascontiguousarray(c[inc])
    out = {"counts": c, "names": names, "labels": labels, "sizes": np.bincount(labels[labels >= 0], minlength=K).astype(np.int64)}
    per = [marker_stats_from_counts(c[:, k, 0], c[:, k, 1], c[:, k, 2], c[:, k, 3] if c.shape[2] == 4 else None) for k in range(K)]
    for key in ("freq", "maf", "het", "call_rate"):
        out[key] = np.stack([p[key] for p in per], axis=1)
    return out


def _fst_windows(L, chrom, pos, window, kb):
    """Window ids per marker (consecutive from 0, cut at chromosome ends) and their table, or (None, None)."""
    if window is None and kb is None:
        return None, None
    ch = np.zeros(L, dtype=np.int64) if chrom is None else np.asarray(chrom, dtype=np.int64).ravel()
    if kb is not None:
        if pos is None:
            raise ValueError("Fst: kb= needs a map with Chr and Pos entries")
        width = int(round(float(kb) * 1000.0))
        if width < 1:
            raise ValueError("Fst: kb must be at least 0.001")
        cell = np.asarray(pos, dtype=np.int64).ravel() // width
    else:
        if int(window) != window or window < 1:
            raise ValueError("Fst: window must be a whole number of at least 1 marker")
        first = np.r_[True, ch[1:] != ch[:-1]]                       # position within the chromosome's run of markers
        start = np.maximum.accumulate(np.where(first, np.arange(L), 0))
        cell = (np.arange(L) - start) // int(window)
    new = np.r_[True, (ch[1:] != ch[:-1]) | (cell[1:] != cell[:-1])]
    wid = np.cumsum(new) - 1
    first_m = np.flatnonzero(new)
    last_m = np.r_[first_m[1:], L] - 1
    return wid, {"chrom": ch[first_m], "first": first_m, "last": last_m}


def _ratio_of_sums(num, den, wid):
    """sum num / sum den over the markers where both are finite; per window when wid is given."""
    ok = np.isfinite(num) & np.isfinite(den)
    nu, de = np.where(ok, num, 0.0), np.where(ok, den, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        if wid is None:
            return np.float64(nu.sum()) / np.float64(de.sum())
        nw = int(wid[-1]) + 1
        return np.bincount(wid, weights=nu, minlength=nw) / np.bincount(wid, weights=de, minlength=nw)


def fst_from_counts(counts, method="hudson", chrom=None, pos=None, window=None, kb=None):
    """Fst from per-group genotype counts alone: counts = integer (L, K, 3) or (L, K, 4) (the first three columns are the called
    genotypes 0 / 1 / 2; p = the frequency of the allele coded 2 among them).  All integer sub-expressions are formed exactly in int64
    (exact for panels of up to 2^30 individuals, the limit of the C ABI), then as few fp64 operations as the formula needs.

    method="hudson" (Bhatia et al. 2013), per pair of groups with allele counts x_k of a_k = 2 called_k:  num = (p1 - p2)^2 -
    p1 (1 - p1) / (a1 - 1) - p2 (1 - p2) / (a2 - 1),  den = p1 (1 - p2) + p2 (1 - p1)  ->  {"pairs": (P, 2) group indices, "num", "den",
    "fst": fp64 (L, P) = num / den, "genome": fp64 (P) = sum num / sum den (the ratio of sums), "matrix": fp64 (K, K) of the latter}.
    method="wc" (Weir and Cockerham 1984) over all r = K groups, n_i called individuals, h_i the observed heterozygote frequency:
    the variance components a, b, c  ->  {"a", "b", "c", "theta": a / (a + b + c), "fis": 1 - c / (b + c): fp64 (L), "genome" =
    sum a / sum (a + b + c), "genome_fis" = 1 - sum c / sum (b + c)}.
    A marker where a group has fewer than 2 called individuals, or whose denominator is zero, is NaN and is left out of every sum.
    window= (markers) or kb= (with pos) adds "windows": {"chrom", "first", "last" (marker indices), "fst" / "theta"}: the ratio of sums per
    window, windows cut at chromosome ends."""
    c = np.asarray(counts).astype(np.int64)
    if c.ndim != 3 or c.shape[2] not in (3, 4) or c.shape[1] < 2:
        raise ValueError("fst_from_counts: counts must be (L, K >= 2, 3 or 4)")
    L, K = c.shape[0], c.shape[1]
    called = c[:, :, 0] + c[:, :, 1] + c[:, :, 2]                    # n_k
    x = 2 * c[:, :, 2] + c[:, :, 1]                                  # copies of the allele coded 2
    a = 2 * called
    wid, wtab = _fst_windows(L, chrom, pos, window, kb)
    f = np.float64
    with np.errstate(divide="ignore", invalid="ignore"):
        if method == "hudson":
            pairs = np.array([(i, j) for i in range(K) for j in range(i + 1, K)], dtype=np.int64)
            num, den = np.full((L, len(pairs)), np.nan), np.full((L, len(pairs)), np.nan)
            for t, (i, j) in enumerate(pairs):
                x1, x2, a1, a2 = x[:, i], x[:, j], a[:, i], a[:, j]
                ok = (called[:, i] >= 2) & (called[:, j] >= 2)
                aa = (a1 * a2).astype(f)
                diff = (x1 * a2 - x2 * a1).astype(f) / aa                                    # p1 - p2
                w1 = (x1 * (a1 - x1)).astype(f) / ((a1 * a1).astype(f) * (a1 - 1).astype(f))     # p1 (1 - p1) / (a1 - 1)
                w2 = (x2 * (a2 - x2)).astype(f) / ((a2 * a2).astype(f) * (a2 - 1).astype(f))
                dint = x1 * (a2 - x2) + x2 * (a1 - x1)
                ok &= dint != 0
                num[:, t] = np.where(ok, diff * diff - w1 - w2, np.nan)
                den[:, t] = np.where(ok, dint.astype(f) / aa, np.nan)
            out = {"pairs": pairs, "num": num, "den": den, "fst": num / den,
                   "genome": np.array([_ratio_of_sums(num[:, t], den[:, t], None) for t in range(len(pairs))])}
            M = np.zeros((K, K))
            M[pairs[:, 0], pairs[:, 1]] = M[pairs[:, 1], pairs[:, 0]] = out["genome"]
            out["matrix"] = M
            if wid is not None:
                out["windows"] = dict(wtab, fst=np.stack([_ratio_of_sums(num[:, t], den[:, t], wid) for t in range(len(pairs))], axis=1))
            return out
        if method != "wc":
            raise ValueError("fst_from_counts: method must be \"hudson\" or \"wc\"")
        r = K
        T, X, H = called.sum(axis=1), x.sum(axis=1), c[:, :, 1].sum(axis=1)
        ok = np.all(called >= 2, axis=1)
        Tf = T.astype(f)
        nbar = Tf / r
        nc = (Tf - (called * called).sum(axis=1).astype(f) / Tf) / (r - 1)
        pbar = X.astype(f) / (2 * T).astype(f)
        hbar = H.astype(f) / Tf
        dev = (x * T[:, None] - X[:, None] * called).astype(f) / (2 * T).astype(f)[:, None]      # n_i (p_i - pbar)
        s2 = (dev * dev / called.astype(f)).sum(axis=1) / ((r - 1) * nbar)
        pq = (X * (2 * T - X)).astype(f) / ((2 * T).astype(f) * (2 * T).astype(f))                # pbar (1 - pbar)
        rr = (r - 1) / f(r)
        va = (nbar / nc) * (s2 - (pq - rr * s2 - hbar / 4) / (nbar - 1))
        vb = (nbar / (nbar - 1)) * (pq - rr * s2 - ((2 * nbar - 1) / (4 * nbar)) * hbar)
        vc = hbar / 2
        tot = va + vb + vc
        ok &= (nc != 0) & (tot != 0)
        va, vb, vc, tot = (np.where(ok, v, np.nan) for v in (va, vb, vc, tot))
        bc = vb + vc
        out = {"a": va, "b": vb, "c": vc, "theta": va / tot, "fis": 1.0 - vc / bc, "genome": _ratio_of_sums(va, tot, None),
               "genome_fis": 1.0 - _ratio_of_sums(vc, bc, None)}
        if wid is not None:
            out["windows"] = dict(wtab, theta=_ratio_of_sums(va, tot, wid), fis=1.0 - _ratio_of_sums(vc, bc, wid))
        return out


def Fst(geno, groups, method="hudson", bed=None, map=None, window=None, kb=None, availmemGb=8, device=0):
    """Fst between the groups of individuals of a panel, per marker and genome-wide -> fst_from_counts' dict (see there for the two
    estimators, Hudson per pair of groups and Weir-Cockerham over all of them, and the NaN rule) plus "names", the group names.  It
    works from GroupCounts' integer counts alone (one pass over the image on the device); bed= counts called genotypes only.
    map (ReadBim's dict) with window= (markers) or kb= adds per-window ratios of sums, cut at chromosome ends."""
    chrom = pos = None
    if map is not None:
        _, _, chrom, pos, _, _, _ = _ld_stats_source("Fst", geno, map, None, None)
    elif kb is not None:
        raise ValueError("Fst: kb= needs a map with Chr and Pos entries")
    gc = GroupCounts(geno, groups, bed=bed, availmemGb=availmemGb, device=device)
    if len(gc["names"]) < 2:
        raise ValueError("Fst: at least two groups are needed")
    out = fst_from_counts(gc["counts"], method=method, chrom=chrom, pos=pos, window=window, kb=kb)
    out["names"] = gc["names"]
    return out


def _chi2_2x2(a, b, c, d):
    """Pearson's chi-square of the 2 x 2 tables (a, b; c, d), int64 arrays: N (ad - bc)^2 / (r1 r2 c1 c2); a zero margin gives NaN."""
    f = np.float64
    N, m1, m2 = a + b + c + d, (a + b) * (c + d), (a + c) * (b + d)
    det = (a * d - b * c).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((m1 != 0) & (m2 != 0), N.astype(f) * (det * det) / (m1.astype(f) * m2.astype(f)), np.nan)


def case_control_from_counts(counts, fisher=None):
    """The case/control association tests of every marker from counts = integer (L, 2, 3 or 4): group 0 the controls, group 1 the cases,
    columns the called genotypes 0 / 1 / 2 (a fourth column, missing, is not used).  With cases (r0, r1, r2), controls (s0, s1, s2),
    n_j = r_j + s_j, R = sum r, S = sum s, N = R + S  ->  {"cases", "controls": the two count rows;  "allelic": the 1-df chi-square of the
    allele table (a, b; c, d) = (2 r2 + r1, 2 r0 + r1; 2 s2 + s1, 2 s0 + s1), "or": a d / (b c);  "trend": Cochran-Armitage with weights
    0, 1, 2, N (N (r1 + 2 r2) - R (n1 + 2 n2))^2 / (R S (N (n1 + 4 n2) - (n1 + 2 n2)^2));  "genotypic": the 2-df Pearson chi-square of the
    2 x 3 table;  "dominant" (genotypes 1 and 2 against 0) and "recessive" (2 against 0 and 1): 1-df;  "p_allelic", "p_trend",
    "p_genotypic", "p_dominant", "p_recessive" by scipy.special.chdtrc;  with fisher= (a function of (L, 4) tables) "p_fisher" of the
    allele table}.  Integer parts are exact in int64 (up to 2^30 individuals), then as few fp64 operations as the formula needs; a zero
    margin gives NaN."""
    from scipy import special
    c = np.asarray(counts).astype(np.int64)
    if c.ndim != 3 or c.shape[1] != 2 or c.shape[2] not in (3, 4):
        raise ValueError("case_control_from_counts: counts must be (L, 2, 3 or 4)")
    f = np.float64
    s0, s1, s2 = c[:, 0, 0], c[:, 0, 1], c[:, 0, 2]
    r0, r1, r2 = c[:, 1, 0], c[:, 1, 1], c[:, 1, 2]
    n0, n1, n2 = r0 + s0, r1 + s1, r2 + s2
    R, S = r0 + r1 + r2, s0 + s1 + s2
    N = R + S
    a, b, cc, d = 2 * r2 + r1, 2 * r0 + r1, 2 * s2 + s1, 2 * s0 + s1
    out = {"cases": c[:, 1, :3].copy(), "controls": c[:, 0, :3].copy(), "allelic": _chi2_2x2(a, b, cc, d)}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["or"] = (a * d).astype(f) / (b * cc).astype(f)
        tnum = (N * (r1 + 2 * r2) - R * (n1 + 2 * n2)).astype(f)
        tvar = N * (n1 + 4 * n2) - (n1 + 2 * n2) * (n1 + 2 * n2)
        tok = (R != 0) & (S != 0) & (tvar != 0)
        out["trend"] = np.where(tok, N.astype(f) * (tnum * tnum) / ((R * S).astype(f) * tvar.astype(f)), np.nan)
        geno = np.zeros(c.shape[0], dtype=f)
        for row, tot in (((r0, r1, r2), R), ((s0, s1, s2), S)):                  # the six cells in a fixed order
            for o, col in zip(row, (n0, n1, n2)):
                dev = (N * o - tot * col).astype(f)                              # N (O - E)
                geno = geno + dev * dev / (N.astype(f) * (tot * col).astype(f))
        out["genotypic"] = np.where((R != 0) & (S != 0) & (n0 != 0) & (n1 != 0) & (n2 != 0), geno, np.nan)
    out["dominant"] = _chi2_2x2(r1 + r2, r0, s1 + s2, s0)
    out["recessive"] = _chi2_2x2(r2, r0 + r1, s2, s0 + s1)
    for key, df in (("allelic", 1), ("trend", 1), ("genotypic", 2), ("dominant", 1), ("recessive", 1)):
        out["p_" + key] = special.chdtrc(float(df), out[key])
    if fisher is not None:
        out["p_fisher"] = fisher(np.stack([a, b, cc, d], axis=1))
    return out


def CaseControl(geno, status, bed=None, fisher=False, availmemGb=8, device=0):
    """Case/control association of every marker of a panel with a binary trait -> case_control_from_counts' dict (the allelic, trend,
    genotypic, dominant and recessive tests and their p-values; see there).  status: one record per individual, 1 = case, 0 = control,
    NaN / None = neither.  The counts come from the device in one pass (rcpp_api.group_counts; with bed= from the .bed file, where a
    missing call is in no cell); fisher=True adds "p_fisher", the exact test of the allele table on the device (rcpp_api.fisher_2x2).
    HWE(out["controls"]) is the Hardy-Weinberg filter among the controls.  Covariates: Logistic; stratified tests are out of scope."""
    st = list(np.asarray(status, dtype=object).ravel())
    lab = np.full(len(st), -1, dtype=np.int32)
    for i, v in enumerate(st):
        if v is None or (isinstance(v, (float, np.floating)) and math.isnan(v)):
            continue
        if v != 0 and v != 1:
            raise ValueError("CaseControl: status must be 1 (case), 0 (control) or NaN / None (neither)")
        lab[i] = int(v)
    n, L, src_bed, bdims, inc = _group_source("CaseControl", geno, bed, None)
    if lab.size != n:
        raise ValueError("CaseControl: %d status records for %d genotyped individuals" % (lab.size, n))
    if src_bed is not None:
        c = rcpp_api.bed_group_counts(src_bed, bdims, lab, 2, availmemGb, device=device)
        c = c if inc is None else np.ascontiguousarray(c[inc])
    else:
        c = rcpp_api.group_counts(geno["asciifileMt"], (n, L), lab, 2, availmemGb, device=device)
    return case_control_from_counts(c, fisher=(lambda t: rcpp_api.fisher_2x2(t, device=device)) if fisher else None)


# ---- max(T) permutation p-values (include/eagle_hip.h section 1b''''vi) ----
def maxt_key64_host(seed, r, N, strata_used=None):
    """key64(r, j), j < N, of section 1b''''vi -> uint64 (N): (stratum << 48) | (h << 16) | j with h the top 32 bits of the splitmix64
    finaliser of seed + (r 2^16 + j + 1) 0x9E3779B97F4A7C15; uint64 arithmetic that wraps."""
    u64 = np.uint64
    N = int(N)
    j = np.arange(N, dtype=u64)
    s = np.zeros(N, dtype=u64) if strata_used is None else np.asarray(strata_used).astype(u64)
    if s.size != N:
        raise ValueError("maxt_key64_host: one stratum per used individual")
    counter = np.full(N, int(r) << 16, dtype=u64) + j + u64(1)
    z = np.full(N, int(seed) & (2 ** 64 - 1), dtype=u64) + counter * u64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
    z = z ^ (z >> u64(31))
    return (s << u64(48)) | ((z >> u64(32)) << u64(16)) | j


def maxt_permutations_host(N, strata_used, seed, first, R):
    """The seeded permutations first .. first + R - 1 of section 1b''''vi restated in numpy -> int32 (R, N), in the form the explicit
    route takes: row q arranges the trait as t'[u_k] = t[u_row[k]].  strata_used: the stratum of every USED individual (None: one
    stratum).  A stable sort of the 64-bit keys (maxt_key64_host); with sigma the order by (stratum, position) and pi the order of the
    keys, row[sigma[k]] = pi[k]."""
    N, R = int(N), int(R)
    s = np.zeros(N, dtype=np.int64) if strata_used is None else np.asarray(strata_used).astype(np.int64)
    sigma = np.argsort(s, kind="stable")
    out = np.empty((R, N), dtype=np.int32)
    for q in range(R):
        out[q, sigma] = np.argsort(maxt_key64_host(seed, int(first) + q, N, strata_used), kind="stable")
    return out


def maxt_digit_planes(t):
    """The int8 planes of the device's operand for integer trait values t (|t| <= 2,097,151) -> (P, planes int8 (P, len(t))): digit p of
    sign(t) (m0 + 128 m1 + 16384 m2), m in [0, 127]; P = 1 up to max |t| = 127, 2 up to 16,383, else 3."""
    tv = np.asarray(t, dtype=np.int64)
    m, sg = np.abs(tv), np.sign(tv)
    mx = int(m.max()) if m.size else 0
    P = 1 if mx <= 127 else (2 if mx <= 16383 else 3)
    return P, np.stack([(sg * ((m >> (7 * p)) & 127)).astype(np.int8) for p in range(P)])


def maxt_host(Mt8, t, used, strata, seed, first, R, perm=None):
    """rcpp_api.maxt restated in numpy: Mt8 = int8 (L, n) of -1 / 0 / +1 (marker-major), t int (n), used a mask or None, strata int (n) or
    None -> the same dict of d_obs, V, key_obs, count1, maxkey, argmax, word for word.  int64 sums (every product is bounded by 2^53,
    checked through _epi_mul), key = (d * d) / V as two fp64 operations."""
    G = np.asarray(Mt8)
    L, n = G.shape
    tv = np.asarray(t, dtype=np.int64).ravel()
    um = np.ones(n, dtype=bool) if used is None else np.asarray(used).astype(bool).ravel()
    u = np.flatnonzero(um)
    N, R = int(u.size), int(R)
    Gu = G[:, u].astype(np.int64)
    tu = tv[u]
    S, Q, T = Gu.sum(axis=1), (Gu * Gu).sum(axis=1), int(tu.sum())
    V = N * Q - S * S
    if perm is None:
        perm = maxt_permutations_host(N, None if strata is None else np.asarray(strata).ravel()[u], seed, first, R)
    perm = np.asarray(perm, dtype=np.int64)
    ST = np.asarray(_epi_mul(S, np.array([T])), dtype=np.int64)

    def keys(c):
        d = np.asarray(_epi_mul(np.array([N]), c), dtype=np.int64) - (ST if c.ndim == 1 else ST[:, None])
        df = d.astype(np.float64)
        Vf = V.astype(np.float64) if c.ndim == 1 else V.astype(np.float64)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return d, np.where(Vf != 0, (df * df) / Vf, 0.0)

    d_obs, key_obs = keys(Gu @ tu)
    count1 = np.zeros(L, dtype=np.int32)
    maxkey, argmax = np.zeros(R, dtype=np.float64), np.zeros(R, dtype=np.int32)
    step = max(1, (1 << 22) // max(L, N))
    for r0 in range(0, R, step):
        d, k = keys(Gu @ tu[perm[r0:r0 + step]].T)
        count1 += (np.abs(d) >= np.abs(d_obs)[:, None]).sum(axis=1).astype(np.int32)
        maxkey[r0:r0 + step], argmax[r0:r0 + step] = k.max(axis=0), k.argmax(axis=0)
    return {"d_obs": d_obs, "V": V, "key_obs": key_obs, "count1": count1, "maxkey": maxkey, "argmax": argmax}


def maxt_from_raw(raw, t_used, kind, scale=1.0, first=1):
    """MaxT's result from the raw outputs (rcpp_api.maxt or maxt_host) and the integer trait of the used individuals.  kind "cc": stat =
    N r^2, the Cochran-Armitage trend chi-square; "qt": stat = (N - 2) r^2 / (1 - r^2), the slope's F(1, N - 2);  r^2 = key / W with W = N
    sum t^2 - T^2 an exact Python int.  count2[m] = #{r : maxkey_r >= key_obs_m} by a sort of maxkey."""
    from scipy import special
    tu = [int(v) for v in np.asarray(t_used).ravel()]
    N, T = len(tu), sum(tu)
    W = N * sum(v * v for v in tu) - T * T
    R = int(raw["maxkey"].size)
    Wf = float(W)

    def stat_of(key):
        r2 = np.asarray(key, dtype=np.float64) / Wf
        if kind == "cc":
            return r2, float(N) * r2
        with np.errstate(divide="ignore", invalid="ignore"):
            return r2, np.where(r2 < 1.0, float(N - 2) * r2 / (1.0 - r2), np.inf)

    ok = raw["V"] != 0
    r2, stat = stat_of(raw["key_obs"])
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = raw["d_obs"].astype(np.float64) / raw["V"].astype(np.float64) / float(scale)
    p = special.chdtrc(1.0, stat) if kind == "cc" else special.fdtrc(1.0, float(N - 2), stat)
    count1 = raw["count1"].astype(np.int64)
    count2 = R - np.searchsorted(np.sort(raw["maxkey"]), raw["key_obs"], side="left").astype(np.int64)
    nan = lambda a: np.where(ok, a, np.nan)                                                    # noqa: E731
    return {"stat": nan(stat), "p": nan(p), "beta": nan(beta), "r2": nan(r2), "count1": count1, "count2": count2,
            "emp1": nan((count1 + 1) / (R + 1.0)), "emp2": nan((count2 + 1) / (R + 1.0)), "max_stat": stat_of(raw["maxkey"])[1],
            "argmax": raw["argmax"].copy(), "n_used": N, "R": R, "kind": kind, "scale": float(scale), "first": int(first),
            "key_obs": raw["key_obs"].copy(), "maxkey": raw["maxkey"].copy(), "V": raw["V"].copy()}


def maxt_merge(a, b):
    """Two MaxT results of one panel, trait and seed over disjoint ranges of permutation ordinals (a second call with first=a["first"] +
    a["R"]) -> the result of the union: count1 add, max_stat / argmax / maxkey concatenate in the order (a, b), count2 and the
    empirical p-values are counted again."""
    if a["kind"] != b["kind"] or a["n_used"] != b["n_used"] or not np.array_equal(a["key_obs"], b["key_obs"]):
        raise ValueError("maxt_merge: the two results are not of one panel and trait")
    if a["first"] + a["R"] > b["first"] and b["first"] + b["R"] > a["first"]:
        raise ValueError("maxt_merge: the ranges of permutation ordinals overlap")
    out = dict(a)
    R = a["R"] + b["R"]
    ok = a["V"] != 0
    out["count1"] = a["count1"] + b["count1"]
    for k in ("max_stat", "argmax", "maxkey"):
        out[k] = np.concatenate([a[k], b[k]])
    out["count2"] = R - np.searchsorted(np.sort(out["maxkey"]), a["key_obs"], side="left").astype(np.int64)
    out["emp1"] = np.where(ok, (out["count1"] + 1) / (R + 1.0), np.nan)
    out["emp2"] = np.where(ok, (out["count2"] + 1) / (R + 1.0), np.nan)
    out["R"], out["first"] = R, min(a["first"], b["first"])
    return out


def maxt_trait(trait, within=None, kind="auto"):
    """MaxT's preparation -> (t int32 (n), used bool (n), strata int32 (n) or None, kind, scale).  A trait of 1 / 0 / NaN is case/control
    ("cc": t = the case indicator); any other is quantitative ("qt": t = quantise_trait of the non-NaN records); NaN / None records are not
    used.  within: any labels (group_labels), the strata of the permutations; a used individual without a label raises ValueError."""
    vals = list(np.asarray(trait, dtype=object).ravel())
    ya = np.array([np.nan if v is None else float(v) for v in vals], dtype=np.float64)
    used = ~np.isnan(ya)
    if not np.all(np.isfinite(ya[used])):
        raise ValueError("MaxT: a trait record is infinite")
    if kind not in ("auto", "cc", "qt"):
        raise ValueError("MaxT: kind must be 'auto', 'cc' or 'qt'")
    binary = bool(np.all((ya[used] == 0) | (ya[used] == 1)))
    if kind == "auto":
        kind = "cc" if binary else "qt"
    if kind == "cc" and not binary:
        raise ValueError("MaxT: a case/control trait must hold 1 (case), 0 (control) or NaN / None (not used)")
    if int(used.sum()) < 3:
        raise ValueError("MaxT: fewer than 3 individuals with a trait record")
    t, scale = np.zeros(ya.size, dtype=np.int32), 1.0
    if kind == "cc":
        t[used] = ya[used].astype(np.int32)
    else:
        t[used], scale = quantise_trait(ya[used])
    if int(t[used].min()) == int(t[used].max()):
        raise ValueError("MaxT: the trait is constant")
    strata = None
    if within is not None:
        lab, names = group_labels(within)
        if lab.size != ya.size:
            raise ValueError("MaxT: within must hold one label per individual (%d)" % ya.size)
        if np.any(lab[used] < 0):
            raise ValueError("MaxT: an individual with a trait record has no label in within")
        if len(names) > 65536:
            raise ValueError("MaxT: more than 65,536 distinct labels in within")
        strata = np.where(used, lab, 0).astype(np.int32)
    return t, used, strata, kind, scale


def MaxT(geno, trait, R=1000, seed=0, within=None, kind="auto", availmemGb=8, device=0, first=1):
    """Permutation p-values of every marker of a panel against one trait (PLINK --assoc --mperm / --model trend --mperm; include/eagle_hip.h
    section 1b''''vi): the R seeded permutations first .. first + R - 1 of the trait among the individuals that have a record, within the
    groups of within= where given (Admixture(...)["assignment"], family ids), all on the device in exact integers.  trait: one record per
    individual (maxt_trait: 1 / 0 / NaN is case/control, anything else quantitative; kind= forces either).
    -> {"stat", "p": the trend chi-square with scipy.special.chdtrc (case/control) or the slope's F(1, N - 2) with fdtrc; "beta" per copy
    of the allele that '2' stands for, in the trait's units, "r2"; "count1", "count2"; "emp1" = (count1 + 1) / (R + 1), the share of
    permutations in which the marker's own statistic reaches the observed one, "emp2" = (count2 + 1) / (R + 1), the share whose largest
    statistic over ALL markers reaches it (family-wise, max(T)); "max_stat" (R) and "argmax" (R): every permutation's largest statistic and
    the lowest marker that attains it; "n_used", "R", "kind", "scale", "first", and "key_obs", "maxkey", "V" (the raw words maxt_merge
    needs)}.  Monomorphic markers (V = 0) have NaN in every statistic and p-value.  A second call with first=first + R continues the run;
    maxt_merge adds two results.  Covariates: pass a residual as the trait."""
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    t, used, strata, kind, scale = maxt_trait(trait, within, kind)
    if t.size != n:
        raise ValueError("MaxT: %d trait records for %d genotyped individuals" % (t.size, n))
    if n > rcpp_api.MAXT_MAX_N:
        raise ValueError("MaxT: more than 65,535 individuals")
    if int(R) < 1 or int(first) < 1:
        raise ValueError("MaxT: R and first must be at least 1")
    raw = rcpp_api.maxt(geno["asciifileMt"], (n, L), t, used=None if used.all() else used, strata=strata, seed=seed, first=first, R=R,
                        availmemGb=availmemGb, device=device)
    return maxt_from_raw(raw, t[used], kind, scale, first)


# ---- transmission disequilibrium test of trios with max(T) flips (include/eagle_hip.h section 1b''''viii) ----
def tdt_families(trios):
    """The families of a trio list that gives no family ids (rule 5 of section 1b''''viii) -> int32 (T): the smallest list position with
    the same (father, mother), so full sibs flip together."""
    tr = np.asarray(trios, dtype=np.int64).reshape(-1, 3)
    first = {}
    return np.asarray([first.setdefault((int(f), int(m)), k) for k, (_, f, m) in enumerate(tr.tolist())], dtype=np.int32)


def tdt_signs_host(family, seed, first, R):
    """The signs of rule 5 -> int64 (R, T): flip first + q gives the trios of family phi the sign -1 when bit 31 of the 32-bit splitmix64
    value at counter = r 2^16 + phi + 1 is set (maxt_key64_host's hash), else +1; uint64 arithmetic that wraps."""
    u64 = np.uint64
    fam = np.asarray(family, dtype=np.int64).ravel().astype(u64)
    r = (np.arange(int(R), dtype=np.int64) + int(first)).astype(u64)
    counter = (r[:, None] << u64(16)) + fam[None, :] + u64(1)
    z = u64(int(seed) & (2 ** 64 - 1)) + counter * u64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
    z = z ^ (z >> u64(31))
    return np.where((z >> u64(63)) != 0, -1, 1).astype(np.int64)


def tdt_host(g, called, trios, family=None, seed=0, first=1, R=0):
    """rcpp_api.tdt / bed_tdt restated in numpy: g = int8 (L, n) with -1 hom A1, 0 het, +1 hom A2, called = bool (L, n) or None (everything
    called; ibd_genotypes_bed gives both from .bed codes), trios = int (T, 3) -> the same dict of trio, marker, key_obs, count1, maxkey,
    argmax, word for word: rules 1 to 5 of include/eagle_hip.h section 1b''''viii by the plane formulas on boolean columns, the flips as
    int64 sums, key = (d * d) / V as two fp64 operations.  tests/tdt_truth.py pins it to loops over allele choices."""
    A, B, Cm = _mendel_planes("tdt_host", g, called)
    L, n = A.shape
    tr, fam, seed, first, R = rcpp_api.tdt_args("tdt_host", trios, n, L, family, seed, first, R)
    T = tr.shape[0]
    tab = np.zeros((T, 6), dtype=np.int32)
    marker = np.zeros((L, 5), dtype=np.int64)
    D = np.zeros((L, T), dtype=np.int64)
    none = np.zeros(L, dtype=bool)
    for k, (c, f, m) in enumerate(tr.tolist()):
        Ac, Bc, Cc = A[:, c], B[:, c], Cm[:, c]
        Af, Bf, Cf = (A[:, f], B[:, f], Cm[:, f]) if f >= 0 else (none, none, none)
        Am, Bm, Cmo = (A[:, m], B[:, m], Cm[:, m]) if m >= 0 else (none, none, none)
        Hc = Cc & ~Ac & ~Bc
        E = (Ac & Bf) | (Bc & Af) | ((Ac | (Hc & Bf)) & Bm) | ((Bc | (Hc & Af)) & Am)
        K = Cc & Cf & Cmo & ~E
        Hf, Hm = Cf & ~Af & ~Bf & K, Cmo & ~Am & ~Bm & K
        PT, PU = Hf & (Bc | (Hc & Am)), Hf & (Ac | (Hc & Bm))
        MT, MU = Hm & (Bc | (Hc & Af)), Hm & (Ac | (Hc & Bf))
        W = Hf & Hm & Hc
        kinds = np.stack([PT, PU, MT, MU, W], axis=1).astype(np.int64)
        cnt = kinds.sum(axis=0)
        tab[k] = (np.count_nonzero(K), np.count_nonzero(Hf), np.count_nonzero(Hm), cnt[0] + cnt[2] + cnt[4], cnt[1] + cnt[3] + cnt[4], cnt[4])
        marker += kinds
        D[:, k] = kinds[:, 0] + kinds[:, 2] - kinds[:, 1] - kinds[:, 3]
    Tm, Um = marker[:, 0] + marker[:, 2] + marker[:, 4], marker[:, 1] + marker[:, 3] + marker[:, 4]
    d_obs, V = Tm - Um, Tm + Um
    Vf = V.astype(np.float64)

    def keys(d):
        df = d.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where((Vf if d.ndim == 1 else Vf[:, None]) != 0, (df * df) / (Vf if d.ndim == 1 else Vf[:, None]), 0.0)

    out = {"trio": tab, "marker": marker.astype(np.int32), "key_obs": keys(d_obs), "count1": np.zeros(L, dtype=np.int32),
           "maxkey": np.zeros(R, dtype=np.float64), "argmax": np.zeros(R, dtype=np.int32)}
    if R >= 1:
        fam = tdt_families(tr) if fam is None else fam
        step = max(1, (1 << 22) // max(L, T))
        for r0 in range(0, R, step):
            d = D @ tdt_signs_host(fam, seed, first + r0, min(step, R - r0)).T
            k = keys(d)
            out["count1"] += (np.abs(d) >= np.abs(d_obs)[:, None]).sum(axis=1).astype(np.int32)
            out["maxkey"][r0:r0 + step], out["argmax"][r0:r0 + step] = k.max(axis=0), k.argmax(axis=0)
    return out


def _tdt_chisq(a, b):
    """(a - b)^2 / (a + b) in fp64 on exact integers, NaN where a + b = 0, and its one-degree-of-freedom p."""
    from scipy import special
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    d, v = (a - b).astype(np.float64), (a + b).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(v != 0, (d * d) / v, np.nan)
    return x, special.chdtrc(1.0, x)


def tdt_summary(raw, first=1):
    """TDT's result from the raw outputs (rcpp_api.tdt, bed_tdt or tdt_host): host fp64 on exact integers.  Per marker: "T" = PT + MT + W
    and "U" = PU + MU + W, the transmissions and non-transmissions of the allele that '2' stands for from het parents; "chisq" = key_obs =
    (T - U)^2 / (T + U) with "p" = scipy.special.chdtrc(1, chisq); "or" = T / U; "p_exact" = min(1, 2 bdtr(min(T, U), T + U, 0.5)), the
    two-sided exact binomial test; "chisq_pat", "p_pat" of (PT, PU) and "chisq_mat", "p_mat" of (MT, MU), where the het x het -> het
    trios (W) cannot take part; "z_poo" = (p1 - p2) / sqrt(p (1 - p) (1 / n1 + 1 / n2)) with p1 = PT / n1, n1 = PT + PU, p2 = MT / n2, n2
    = MT + MU and p = (PT + MT) / (n1 + n2), the pooled two-proportion z of paternal against maternal transmission, and "p_poo" =
    2 ndtr(-|z_poo|) (this formula and no other program's).  With flips: "count1", "count2", "emp1" = (count1 + 1) / (R + 1) and "emp2"
    = (count2 + 1) / (R + 1) as MaxT defines them, "max_stat" = maxkey and "argmax".  Markers without an informative transmission
    (T + U = 0) have NaN in every statistic and p-value.  "R", "first", and "marker", "key_obs", "maxkey", "trio" (the raw words
    tdt_merge needs)."""
    from scipy import special
    mk = np.asarray(raw["marker"]).astype(np.int64)
    PT, PU, MT, MU, W = (mk[:, j] for j in range(5))
    T, U = PT + MT + W, PU + MU + W
    V = T + U
    ok = V != 0
    nan = lambda a: np.where(ok, a, np.nan)                                                    # noqa: E731
    chisq = np.asarray(raw["key_obs"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        odds = np.where(U != 0, T / U.astype(np.float64), np.where(T != 0, np.inf, np.nan))
        n1, n2 = (PT + PU).astype(np.float64), (MT + MU).astype(np.float64)
        p1, p2, pp = PT / n1, MT / n2, (PT + MT) / (n1 + n2)
        z = (p1 - p2) / np.sqrt(pp * (1.0 - pp) * (1.0 / n1 + 1.0 / n2))
    z = np.where(np.isfinite(z), z, np.nan)
    cp, pp_ = _tdt_chisq(PT, PU)
    cm, pm = _tdt_chisq(MT, MU)
    R = int(np.asarray(raw["maxkey"]).size)
    out = {"T": T, "U": U, "chisq": nan(chisq), "p": nan(special.chdtrc(1.0, chisq)), "or": odds,
           "p_exact": nan(np.minimum(1.0, 2.0 * special.bdtr(np.minimum(T, U).astype(np.float64), V, 0.5))),
           "chisq_pat": cp, "p_pat": pp_, "chisq_mat": cm, "p_mat": pm, "z_poo": z, "p_poo": 2.0 * special.ndtr(-np.abs(z)),
           "R": R, "first": int(first), "marker": np.asarray(raw["marker"]).copy(), "key_obs": chisq.copy(),
           "maxkey": np.asarray(raw["maxkey"]).copy(), "trio": np.asarray(raw["trio"]).copy()}
    if R >= 1:
        count1 = np.asarray(raw["count1"]).astype(np.int64)
        count2 = R - np.searchsorted(np.sort(raw["maxkey"]), chisq, side="left").astype(np.int64)
        out.update({"count1": count1, "count2": count2, "emp1": nan((count1 + 1) / (R + 1.0)), "emp2": nan((count2 + 1) / (R + 1.0)),
                    "max_stat": np.asarray(raw["maxkey"]).copy(), "argmax": np.asarray(raw["argmax"]).copy()})
    return out


def tdt_merge(a, b):
    """Two TDT results of one panel, trio list and seed over disjoint ranges of flip ordinals (a second call with first=a["first"] +
    a["R"]) -> the result of the union: count1 add, max_stat / argmax / maxkey concatenate in the order (a, b), count2 and the empirical
    p-values are counted again."""
    if not np.array_equal(a["marker"], b["marker"]) or not np.array_equal(a["trio"], b["trio"]):
        raise ValueError("tdt_merge: the two results are not of one panel and trio list")
    if a["R"] < 1 or b["R"] < 1:
        raise ValueError("tdt_merge: a result without flips")
    if a["first"] + a["R"] > b["first"] and b["first"] + b["R"] > a["first"]:
        raise ValueError("tdt_merge: the ranges of flip ordinals overlap")
    raw = {"marker": a["marker"], "trio": a["trio"], "key_obs": a["key_obs"], "count1": a["count1"] + b["count1"],
           "maxkey": np.concatenate([a["maxkey"], b["maxkey"]]), "argmax": np.concatenate([a["argmax"], b["argmax"]])}
    return tdt_summary(raw, min(a["first"], b["first"]))


def TDT(geno, trios=None, fam=None, affected=None, bed=None, include=None, map=None, R=0, seed=0, family=None, first=1, availmemGb=8, device=0):
    """The transmission disequilibrium test of the parent-offspring trios of a pedigreed panel (Spielman 1993; include/eagle_hip.h section
    1b''''viii; rcpp_api.tdt; what PLINK reports as --tdt, --tdt poo and --tdt mperm, agreement with that program is not claimed; every
    marker is taken as autosomal): do het parents pass the allele that '2' stands for to their affected children more often than not?
    Unlike CaseControl on the children it is immune to population stratification.  -> tdt_summary's dict, plus "trios": the int32 (T, 3)
    trios that were used and, with a map, "SNP".
    trios = int (T, 3) of (child, father, mother), or fam = a .fam file (or ReadFam's dict) whose recorded trios are used (fam_trios;
    default: the .fam of bed), as Mendel finds them.  affected: a bool per individual; default the .fam phenotype '2' when a .fam is
    read, and everybody when trios= is given.  Only trios with an affected child are used; ValueError if none is left.  A trio with an
    unknown parent, a missing call or a Mendel error at a marker contributes nothing there.
    R >= 1: R seeded flips of transmitted and untransmitted alleles within families (family: one whole number in [0, 65535] per trio of
    the list, before the affected children are selected; default: trios with the same parents), giving emp1 and the family-wise emp2 as MaxT does; first=first + R continues a run and
    tdt_merge adds two results.  At most 65,535 trios with flips.
    On the ingested (het-filled) panel a missing call is a het, which invents informative parents; bed = the .bed file (or prefix) the
    panel was ingested from is the route for un-imputed panels (rcpp_api.bed_tdt); include = the panel's markers in the file, default
    geno's marker_index."""
    n, L, _, _, src_bed, bdims, inc = _ld_stats_source("TDT", geno, map, bed, include)
    aff = None
    if trios is None:
        if fam is None and src_bed is None:
            raise ValueError("TDT: give trios=, fam= or bed=")
        fam = bed_fileset(src_bed)[2] if fam is None else fam
        famd = ReadFam(fam) if isinstance(fam, (str, os.PathLike)) else fam
        if len(famd["IID"]) != n:
            raise ValueError("TDT: the .fam names %d individuals, the panel holds %d" % (len(famd["IID"]), n))
        trios = fam_trios(famd)
        if trios.shape[0] == 0:
            raise ValueError("TDT: the .fam records no parent")
        aff = np.asarray([p == "2" for p in famd["Pheno"]], dtype=bool)
    tr = rcpp_api.mendel_trios("TDT", trios, n)
    if affected is not None:
        aff = np.asarray(affected)
        if aff.dtype != bool or aff.shape != (n,):
            raise ValueError("TDT: affected must be one bool per individual (%d)" % n)
    if family is not None:
        family = np.asarray(family)
        if family.shape != (tr.shape[0],):
            raise ValueError("TDT: family must hold one entry per trio of the list (%d)" % tr.shape[0])
    if aff is not None:
        use = aff[tr[:, 0]]
        family = None if family is None else family[use]
        tr = np.ascontiguousarray(tr[use])
    if tr.shape[0] == 0:
        raise ValueError("TDT: no trio with an affected child is left")
    if src_bed is None:
        raw = rcpp_api.tdt(geno["asciifileM"], (n, L), tr, family, seed, first, R, availmemGb, device=device)
    else:
        raw = rcpp_api.bed_tdt(src_bed, bdims, tr, inc, family, seed, first, R, availmemGb, device=device)
    out = tdt_summary(raw, first)
    out["trios"] = tr
    if map is not None and "SNP" in map:
        out["SNP"] = list(map["SNP"])
    return out


# ---- logistic regression per marker with covariates, Firth fallback (include/eagle_hip.h section 1b''''iv) ----
_LOGIT_ETA_MAX, _LOGIT_STEP_MAX, _LOGIT_PIVOT_REL = 40.0, 5.0, 2.0 ** -40


def _logit_eval(Xt, y, beta):
    """One evaluation of section 1b''''iv at beta over the rows of Xt (used individuals only): (mu, y - mu, w, U, I, loglik, max |eta|)."""
    eta = Xt @ beta
    e = np.exp(-np.abs(eta))
    d = 1.0 / (1.0 + e)
    mu = np.where(eta >= 0.0, d, e * d)
    w = e * d * d
    ll = float(np.sum(y * eta - (np.maximum(eta, 0.0) + np.log1p(e))))
    res = np.where(y > 0.5, np.where(eta >= 0.0, e * d, d), -mu)                    # y - mu without cancellation
    return mu, res, w, Xt.T @ res, Xt.T @ (w[:, None] * Xt), ll, float(np.max(np.abs(eta)))


def _logit_chol(A):
    """The lower Cholesky factor of A column by column, or None when a pivot is not finite or not above 2^-40 of its diagonal entry."""
    p = A.shape[0]
    Lm = np.tril(A).astype(np.float64)
    d0 = np.diag(A).copy()
    for j in range(p):
        d = Lm[j, j]
        if not (d > d0[j] * _LOGIT_PIVOT_REL) or not (d < np.inf):
            return None
        l = math.sqrt(d)
        Lm[j, j] = l
        Lm[j + 1:, j] /= l
        for k in range(j + 1, p):
            Lm[k:, k] -= Lm[k:, j] * Lm[k, j]
    return Lm


def _logit_solve(Lm, b):
    from scipy.linalg import solve_triangular
    return solve_triangular(Lm, solve_triangular(Lm, b, lower=True), lower=True, trans="T")


def _logit_fit(Xt, y, start, firth, tol, max_iter, score=None):
    """One fit of section 1b''''iv from `start` -> (gamma, se, score, loglik, code, evaluations), gamma the LAST parameter."""
    nan = float("nan")
    beta = np.array(start, dtype=np.float64)
    g = beta.size - 1
    ev = 0
    with np.errstate(all="ignore"):
        while ev < max_iter:
            mu, res, w, U, I, ll, mx = _logit_eval(Xt, y, beta)
            ev += 1
            Lm = _logit_chol(I)
            if Lm is None:
                return nan, nan, nan if score is None else score, nan, 2, ev
            if ev == 1 and score is None:
                score = float(U[g] * U[g] / (Lm[g, g] * Lm[g, g]))
            if not firth and mx > _LOGIT_ETA_MAX:
                return nan, nan, score, nan, 3, ev
            if firth:
                Inv = _logit_solve(Lm, np.eye(beta.size))
                h = w * np.einsum("ij,jk,ik->i", Xt, Inv, Xt)
                U = Xt.T @ (res + h * (0.5 - mu))
            delta = _logit_solve(Lm, U)
            md = float(np.max(np.abs(delta))) if np.all(np.isfinite(delta)) else nan
            if md > _LOGIT_STEP_MAX:
                delta = delta * (_LOGIT_STEP_MAX / md)
            beta = beta + delta
            if md <= tol:
                return float(beta[g]), 1.0 / float(Lm[g, g]), score, ll, 0, ev
    return nan, nan, nan if score is None else score, nan, 1, ev


def logistic_null_host(X, y, tol=1e-10, max_iter=50):
    """The covariates-only logistic fit of y (0 / 1) on the columns of X (every row used) -> beta0 fp64 (c): numpy fp64 Newton with the
    step cap and the stop rule of include/eagle_hip.h section 1b''''iv, from beta = 0.  ValueError when it does not get there."""
    Xt, yv = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel()
    if Xt.ndim != 2 or Xt.shape[0] != yv.size or Xt.shape[1] < 1:
        raise ValueError("logistic_null_host: X must be (n, c) with one row per entry of y")
    beta = np.zeros(Xt.shape[1])
    for _ in range(int(max_iter)):
        _, _, _, U, I, _, _ = _logit_eval(Xt, yv, beta)
        Lm = _logit_chol(I)
        if Lm is None:
            raise ValueError("logistic_null_host: the covariates are collinear among the used individuals")
        delta = _logit_solve(Lm, U)
        md = float(np.max(np.abs(delta)))
        if md > _LOGIT_STEP_MAX:
            delta = delta * (_LOGIT_STEP_MAX / md)
        beta = beta + delta
        if md <= tol:
            return beta
    raise ValueError("logistic_null_host: the covariates-only fit did not converge (separated by the covariates?)")


def logistic_host(Mt8, status, X, firth=2, tol=1e-10, max_iter=50, beta0=None):
    """rcpp_api.logistic restated in numpy, marker by marker: Mt8 = int8 (L, n) of -1 / 0 / +1 (marker-major), status in {-1, 0, 1}, X
    (n, c) -> (stat (L, 4), info (L, 2)) by the rule of include/eagle_hip.h section 1b''''iv.  Not bit-equal to the device (exp, log1p
    and the order of the sums differ); tests/logistic_truth.py holds both to 40-digit roots."""
    G = np.asarray(Mt8)
    sv = np.asarray(status).astype(np.int64).ravel()
    Xa = np.asarray(X, dtype=np.float64)
    used = sv >= 0
    Xu, y = Xa[used], sv[used].astype(np.float64)
    b0 = logistic_null_host(Xu, y, tol, max_iter) if beta0 is None else np.asarray(beta0, dtype=np.float64).ravel()
    start = np.concatenate([b0, [0.0]])
    stat, info = np.full((G.shape[0], 4), np.nan), np.zeros((G.shape[0], 2), dtype=np.int32)
    for m in range(G.shape[0]):
        Xt = np.column_stack([Xu, G[m, used].astype(np.float64) + 1.0])
        if firth == 1:
            r = _logit_fit(Xt, y, start, True, tol, max_iter)
            r = r[:4] + (r[4] + 256, r[5])
        else:
            r = _logit_fit(Xt, y, start, False, tol, max_iter)
            if firth == 2 and r[4] != 0 and not (r[4] == 2 and r[5] == 1):
                r = _logit_fit(Xt, y, start, True, tol, max_iter, score=r[2])
                r = r[:4] + (r[4] + 256, r[5])
        stat[m], info[m] = r[:4], r[4:]
    return stat, info


_LOGIT_FIRTH = {"ml": 0, "none": 0, False: 0, 0: 0, "firth": 1, True: 1, 1: 1, "fallback": 2, 2: 2}


def Logistic(geno, status, X=None, firth="fallback", tol=1e-10, max_iter=50, availmemGb=8, device=0):
    """Case/control association of every marker of a panel with covariates: the logistic fit  logit P(case) = x' beta + g gamma  per
    marker on the device (rcpp_api.logistic; include/eagle_hip.h section 1b''''iv) -> {"beta": gamma per allele copy of the '2'
    character (the allele whose odds ratio CaseControl reports), "se", "or" = exp(beta), "z" = beta / se, "p": two-sided Wald
    (scipy.special.ndtr), "score": the score test of gamma = 0 and "p_score" (chdtrc, 1 df; with X=None the trend test of CaseControl),
    "lrt" = 2 (l - l0) and "p_lrt" for maximum-likelihood fits (NaN under Firth), "code", "iterations", "firth": bool per marker,
    "n_used", "beta0": the covariates-only fit}.  status as in CaseControl: 1 = case, 0 = control, NaN / None = not used.  X: (n, c <=
    15) covariates WITH the intercept column, e.g. what am.add_pcs(X, pca) returns; None = intercept only; an individual with a NaN
    covariate is not used.  firth: "fallback" (Firth's penalised fit where ML fails: separation, no convergence), "firth" (every marker)
    or "ml".  A missing call of the source is a heterozygote on the image, as everywhere else: impute first (ReadMarker(..., impute=k))
    where that matters; there is no .bed route."""
    from scipy import special
    if firth not in _LOGIT_FIRTH:
        raise ValueError("Logistic: firth must be \"fallback\", \"firth\" or \"ml\"")
    st = list(np.asarray(status, dtype=object).ravel())
    sv = np.full(len(st), -1, dtype=np.int32)
    for i, v in enumerate(st):
        if v is None or (isinstance(v, (float, np.floating)) and math.isnan(v)):
            continue
        if v != 0 and v != 1:
            raise ValueError("Logistic: status must be 1 (case), 0 (control) or NaN / None (not used)")
        sv[i] = int(v)
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    if sv.size != n:
        raise ValueError("Logistic: %d status records for %d genotyped individuals" % (sv.size, n))
    Xa = np.ones((n, 1)) if X is None else np.asarray(X, dtype=np.float64)
    if Xa.ndim == 1:
        Xa = Xa[:, None]
    if Xa.ndim != 2 or Xa.shape[0] != n or not 1 <= Xa.shape[1] <= rcpp_api.LOGISTIC_MAX_COVARIATES:
        raise ValueError("Logistic: X must be (%d, c) with 1 <= c <= %d, the intercept column included" % (n, rcpp_api.LOGISTIC_MAX_COVARIATES))
    if np.any(np.isinf(Xa)):
        raise ValueError("Logistic: X holds an infinite entry")
    sv[np.any(np.isnan(Xa), axis=1)] = -1
    used = sv >= 0
    if not (sv == 1).any() or not (sv == 0).any():
        raise ValueError("Logistic: no case or no control among the used individuals")
    y = sv[used].astype(np.float64)
    b0 = logistic_null_host(Xa[used], y, tol, max_iter)
    ll0 = _logit_eval(Xa[used], y, b0)[5]
    stat, info = rcpp_api.logistic(geno["asciifileMt"], (n, L), sv, Xa, b0, _LOGIT_FIRTH[firth], tol, max_iter, availmemGb, device=device)
    beta, se, score, ll = stat[:, 0], stat[:, 1], stat[:, 2], stat[:, 3]
    is_firth = info[:, 0] >= 256
    with np.errstate(all="ignore"):
        z = beta / se
        lrt = np.where(is_firth, np.nan, 2.0 * (ll - ll0))
        return {"beta": beta.copy(), "se": se.copy(), "or": np.exp(beta), "z": z, "p": 2.0 * special.ndtr(-np.abs(z)), "score": score.copy(),
                "p_score": special.chdtrc(1.0, score), "lrt": lrt, "p_lrt": special.chdtrc(1.0, np.maximum(lrt, 0.0)),
                "code": info[:, 0].copy(), "iterations": info[:, 1].copy(), "firth": is_firth, "n_used": int(used.sum()), "beta0": b0}


# ---------------------------------------------------------------------------------------------------------------------------
# Admixture: model-based ancestry proportions (include/eagle_hip.h section 1b''''v; device: rcpp_api.admixture_em).
# ---------------------------------------------------------------------------------------------------------------------------
ADMIX_EPS, ADMIX_KMAX = rcpp_api.ADMIX_EPS, rcpp_api.ADMIX_KMAX


def _admix_loglik(D, P, Pb):
    """sum d ln p + (2 - d) ln pbar, a term with a zero factor being 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sum(np.where(D > 0, D * np.log(P), 0.0) + np.where(D < 2, (2.0 - D) * np.log(Pb), 0.0)))


def admixture_host(Mt8, Q, F, steps=1):
    """rcpp_api.admixture_em restated in numpy: Mt8 = int8 (L, n) of -1 / 0 / +1 (marker-major), Q (n, K), F (L, K) -> (Q, F, loglik
    (steps + 1)) by the rule of include/eagle_hip.h section 1b''''v.  Not bit-equal to the device (the order of the sums and log
    differ); tests/admixture_truth.py holds both to 40-digit arithmetic."""
    D = np.asarray(Mt8).T.astype(np.float64) + 1.0                     # (n, L) dosages
    Q, F = np.array(Q, dtype=np.float64), np.array(F, dtype=np.float64)
    twoL = 2.0 * D.shape[1]
    ll = np.zeros(int(steps) + 1)
    for t in range(int(steps) + 1):
        Fb = 1.0 - F
        P, Pb = Q @ F.T, Q @ Fb.T                                      # p-bar is its own sum
        ll[t] = _admix_loglik(D, P, Pb)
        if t == steps:
            break
        A, B = D / P, (2.0 - D) / Pb
        sa, sb = F * (A.T @ Q), Fb * (B.T @ Q)
        tot = sa + sb
        with np.errstate(divide="ignore", invalid="ignore"):
            Fn = np.where(tot > 0.0, sa / tot, F)
        T = Q * (A @ F + B @ Fb)
        Qn = np.maximum(T / twoL, ADMIX_EPS)
        Q, F = Qn / Qn.sum(axis=1, keepdims=True), np.clip(Fn, ADMIX_EPS, 1.0 - ADMIX_EPS)
    return Q, F, ll


def admixture_init(n, L, K, seed, freq=None):
    """A start for Admixture: Q (n, K) one Dirichlet(1) draw per individual, F (L, K) the marker's frequency (freq, L values; 0.5
    when None) plus a uniform jitter in [-0.1, 0.1] per population, clipped to [0.05, 0.95].  Both from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    Q = rng.dirichlet(np.ones(int(K)), size=int(n))
    f = np.full(int(L), 0.5) if freq is None else np.asarray(freq, dtype=np.float64).ravel()
    if f.size != L:
        raise ValueError("admixture_init: freq must hold one frequency per marker (%d)" % L)
    F = np.clip(f[:, None] + rng.uniform(-0.1, 0.1, size=(int(L), int(K))), 0.05, 0.95)
    return Q / Q.sum(axis=1, keepdims=True), F


def _admix_project(Q, F):
    Q = np.maximum(Q, ADMIX_EPS)
    return Q / Q.sum(axis=1, keepdims=True), np.clip(F, ADMIX_EPS, 1.0 - ADMIX_EPS)


def Admixture(geno, K, seed=0, tol=1e-4, max_iter=2000, accel="squarem", init=None, availmemGb=8, device=0, step=None):
    """Model-based ancestry proportions of a panel for K ancestral populations: EM on the likelihood of FRAPPE / ADMIXTURE / STRUCTURE,
    every step on the device (rcpp_api.admixture_em; include/eagle_hip.h section 1b''''v) -> {"Q" (n, K): the fractions of every
    individual, "F" (K, L): the frequency of the '2' character's allele in every population, "loglik": the trace, one entry per EM step
    evaluated (it never falls), "iterations" = len(loglik) - 1, "converged", "K", "assignment" = argmax_k Q: a groups= argument for
    Fst and GroupCounts}.  The components are ordered by decreasing mean of Q, so a relabelling of the start does not reach the caller;
    am.add_ancestry appends Q's columns to a design matrix.
    accel="squarem" (Varadhan and Roland 2008): a cycle takes two EM steps theta0 -> theta1 -> theta2, r = theta1 - theta0,
    v = theta2 - theta1 - r, alpha = min(-1, -|r| / |v|), theta' = theta0 - 2 alpha r + alpha^2 v projected (F clipped, Q floored and
    renormalised), then one stabilising EM step from theta', whose first likelihood is l(theta'); where l(theta') < l(theta2) the cycle
    falls back to theta2.  accel="none" is plain EM.  Either stops when a cycle (a step) raises the log-likelihood by less than tol,
    or after max_iter EM steps.  init: (Q, F (L, K)) or None = admixture_init(n, L, K, seed, the markers' frequencies).  step: a
    callable with rcpp_api.admixture_em's shape to run instead of it (admixture_host on a CPU).  A missing call of the source is a
    heterozygote on the image: impute first where that matters.  Supervised mode and cross-validation of K are out of scope."""
    if accel not in ("squarem", "none"):
        raise ValueError("Admixture: accel must be \"squarem\" or \"none\"")
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= ADMIX_KMAX:
        raise ValueError("Admixture: K must be a whole number in [1, %d]" % ADMIX_KMAX)
    if not tol > 0.0 or isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1:
        raise ValueError("Admixture: tol must be positive and max_iter a whole number of at least 1")
    K, max_iter = int(K), int(max_iter)
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    fMt, dims = geno["asciifileMt"], (n, L)
    if init is None:
        freq = None
        if step is None:
            c = rcpp_api.marker_counts(fMt, dims, availmemGb, device=device).astype(np.float64)
            freq = (c[:, 1] + 2.0 * c[:, 2]) / (2.0 * n)
        Q, F = admixture_init(n, L, K, seed, freq)
    else:
        Q, F = rcpp_api._admixture_inputs("Admixture", n, L, init[0], init[1], 1)
        if Q.shape[1] != K:
            raise ValueError("Admixture: init holds %d components, K = %d" % (Q.shape[1], K))
    if step is None:
        def step(f, d, Q, F, steps=1):
            return rcpp_api.admixture_em(f, d, Q, F, steps, availmemGb, device=device)
    trace, converged = [], False
    if accel == "none":
        while len(trace) - 1 < max_iter and not converged:
            todo = min(8, max_iter - max(len(trace) - 1, 0))
            Q, F, ll = step(fMt, dims, Q, F, todo)
            trace.extend(ll if not trace else ll[1:])
            converged = bool(np.any(np.diff(ll) < tol))
    else:
        while not converged:
            if len(trace) - 1 + 3 > max_iter and trace:
                break
            Q1, F1, la = step(fMt, dims, Q, F, 1)
            Q2, F2, lb = step(fMt, dims, Q1, F1, 1)
            if not trace:
                trace.append(float(la[0]))
            l0 = trace[-1]
            trace.extend([float(la[1]), float(lb[1])])
            rq, rf = Q1 - Q, F1 - F
            vq, vf = Q2 - Q1 - rq, F2 - F1 - rf
            nr = math.sqrt(float(np.sum(rq * rq) + np.sum(rf * rf)))
            nv = math.sqrt(float(np.sum(vq * vq) + np.sum(vf * vf)))
            if nv == 0.0:                                              # the map is linear here: nothing to extrapolate
                Q, F, converged = Q2, F2, True
                break
            alpha = min(-1.0, -nr / nv)
            Qp, Fp = _admix_project(Q - 2.0 * alpha * rq + alpha * alpha * vq, F - 2.0 * alpha * rf + alpha * alpha * vf)
            Q3, F3, lc = step(fMt, dims, Qp, Fp, 1)
            if lc[0] < lb[1] or not np.isfinite(lc[1]):                # the extrapolation lost ground: theta2 stands
                Q, F = Q2, F2
                trace.append(float(lb[1]))
            else:
                Q, F = Q3, F3
                trace.append(float(lc[1]))
            converged = trace[-1] - l0 < tol
    order = np.argsort(-Q.mean(axis=0), kind="stable")
    Q, F = np.ascontiguousarray(Q[:, order]), np.ascontiguousarray(F[:, order].T)
    return {"Q": Q, "F": F, "loglik": np.asarray(trace, dtype=np.float64), "iterations": len(trace) - 1, "converged": bool(converged), "K": K,
            "assignment": np.argmax(Q, axis=1)}


# ---------------------------------------------------------------------------------------------------------------------------
# The exact per-marker mixed-model test (include/eagle_hip.h section 1d'; device: rcpp_api.spectral_lmm, am.GWAS).
# ---------------------------------------------------------------------------------------------------------------------------
LMM_THETA_MIN, LMM_THETA_MAX, LMM_STEP_MAX, LMM_PIVOT_REL = -10.0, 10.0, 2.0, 2.0 ** -40


def _lmm_eval(lam, B, n, reml, theta):
    """One evaluation of section 1d' at theta for B = [U^T X | z | U^T y] (n x (p + 1)) -> None (singular) or dict(g, gp, R, gamma,
    ipp = (A_1^-1)_pp, L = the Cholesky factor of A_1, delta)."""
    p = B.shape[1] - 1
    delta = math.exp(theta)
    w = 1.0 / (lam + delta)
    w2 = w * w
    w3 = w2 * w
    S1, S2, S3 = B.T @ (w[:, None] * B), B.T @ (w2[:, None] * B), B.T @ (w3[:, None] * B)
    Lm = _logit_chol(S1[:p, :p])                                                      # the pivot rule, LMM_PIVOT_REL = 2^-40
    if Lm is None:
        return None
    b1, b2, b3 = S1[:p, p], S2[:p, p], S3[:p, p]
    beta = _logit_solve(Lm, b1)
    R = S1[p, p] - b1 @ beta
    if not (R > S1[p, p] * LMM_PIVOT_REL) or not (R < np.inf):
        return None
    a2, a3 = S2[:p, :p] @ beta, S3[:p, :p] @ beta
    Q = S2[p, p] + beta @ (a2 - 2.0 * b2)
    W3 = S3[p, p] + beta @ (a3 - 2.0 * b3)
    u = b2 - a2
    C = W3 - u @ _logit_solve(Lm, u)
    Inv = _logit_solve(Lm, np.eye(p))
    if reml:
        M = Inv @ S2[:p, :p]
        m, T, T2 = n - p, w.sum() - np.sum(Inv * S2[:p, :p]), w2.sum() - 2.0 * np.sum(Inv * S3[:p, :p]) + np.sum(M * M.T)
    else:
        m, T, T2 = n, w.sum(), w2.sum()
    qr = Q / R
    g = delta * 0.5 * (m * qr - T)
    gp = g + delta * delta * 0.5 * (m * (qr * qr - 2.0 * C / R) + T2)
    if not (np.isfinite(g) and np.isfinite(gp)):
        return None
    return {"g": float(g), "gp": float(gp), "R": float(R), "gamma": float(beta[p - 1]), "ipp": float(Inv[p - 1, p - 1]), "L": Lm, "delta": delta}


def _lmm_fit(lam, B, reml, theta0, tol, max_iter):
    """The iteration of section 1d' for one marker -> (gamma, se, delta, vg, ll, code, iterations)."""
    n, p = B.shape[0], B.shape[1] - 1
    nan = float("nan")
    theta, lo, hi, have_lo, have_hi, it = float(theta0), LMM_THETA_MIN, LMM_THETA_MAX, False, False, 0
    with np.errstate(all="ignore"):
        while True:
            E = _lmm_eval(lam, B, n, reml, theta)
            if E is None:
                return nan, nan, nan, nan, nan, 2, it
            g, gp = E["g"], E["gp"]
            if g > 0.0:
                lo, have_lo = theta, True
            if g < 0.0:
                hi, have_hi = theta, True
            if g > 0.0 and theta >= LMM_THETA_MAX:
                code = 4
                break
            if g < 0.0 and theta <= LMM_THETA_MIN:
                code = 3
                break
            t = theta - g / gp if gp != 0.0 else nan
            if not (gp < 0.0 and lo < t < hi and abs(t - theta) <= LMM_STEP_MAX):
                if (g > 0.0 and have_hi) or (g < 0.0 and have_lo):
                    t = 0.5 * (lo + hi)
                elif g > 0.0:
                    t = min(theta + LMM_STEP_MAX, LMM_THETA_MAX)
                elif g < 0.0:
                    t = max(theta - LMM_STEP_MAX, LMM_THETA_MIN)
                else:
                    t = theta
            if abs(t - theta) <= tol:
                code = 0
                break
            if it >= max_iter:
                code = 1
                break
            theta = t
            it += 1
        m = n - p if reml else n
        vg = E["R"] / m
        ll = m * (math.log(m / (2.0 * math.pi)) - 1.0 - math.log(E["R"])) - float(np.sum(np.log(lam + E["delta"])))
        if reml:
            ll -= 2.0 * float(np.sum(np.log(np.diag(E["L"]))))
        return E["gamma"], math.sqrt(vg * E["ipp"]), E["delta"], vg, 0.5 * ll, code, it


def lmm_host(lam, UtX, Uty, Zrows, reml=True, theta0=None, tol=1e-10, max_iter=50):
    """rcpp_api.spectral_lmm restated in numpy, marker by marker, by the rule of include/eagle_hip.h section 1d': lam (n) the
    eigenvalues of K, UtX = U^T X (n x c, the intercept column included), Uty = U^T y, Zrows (L x n): row i = U^T m_i, what
    spectral_rows returns transposed -> (stat (L, 5) = gamma, se, delta, vg, ll; info (L, 2) = code, iterations).  theta0: ln delta of
    the null fit; None: emma_REMLE_eig (reml) / emma_MLE_eig on X alone.  Not bit-equal to the device (exp, log and the order of the
    sums differ); tests/lmm_truth.py holds both to 40-digit roots."""
    lam = np.asarray(lam, dtype=np.float64).ravel()
    n = lam.size
    Ut = np.asarray(UtX, dtype=np.float64).reshape(n, -1)
    ut = np.asarray(Uty, dtype=np.float64).ravel()
    Zr = np.asarray(Zrows, dtype=np.float64).reshape(-1, n)
    c = Ut.shape[1]
    if not 1 <= c <= 14 or ut.size != n or n <= c + 2:
        raise ValueError("lmm_host: UtX must be (n, c) with 1 <= c <= 14 and n > c + 2, Uty of length n")
    if not (0.0 < tol < 1.0) or not 0 <= int(max_iter) <= 1000:
        raise ValueError("lmm_host: tol in (0, 1) and max_iter in [0, 1000]")
    if theta0 is None:
        from . import am
        theta0 = math.log((am.emma_REMLE_eig if reml else am.emma_MLE_eig)(lam, Ut, ut)["delta"])
    theta0 = min(max(float(theta0), LMM_THETA_MIN), LMM_THETA_MAX)
    stat, info = np.full((Zr.shape[0], 5), np.nan), np.zeros((Zr.shape[0], 2), dtype=np.int32)
    for i in range(Zr.shape[0]):
        r = _lmm_fit(lam, np.column_stack([Ut, Zr[i], ut]), bool(reml), theta0, tol, int(max_iter))
        stat[i], info[i] = r[:5], r[5:]
    return stat, info


def GWAS(trait, X, geno, exact="all", method="reml", p_exact=None, map=None, backend=None, availmemGb=8, device=0, Zmat=None):
    """The single-locus mixed-model scan of a quantitative trait, y = X beta + m_i gamma + g + e for every marker i (am.GWAS): the P3D /
    EMMAX score test of every marker from one pass over the resident Z ("score", "p_score", "beta_p3d") and the exact test with delta
    re-estimated per marker on the device (include/eagle_hip.h section 1d': "beta", "se", "stat", "p", "delta", "vg", "ve", "ll", "code",
    "iterations") for every marker (exact="all"), none (exact="none") or those with p_score < p_exact.  method="reml": Wald F test;
    "ml": likelihood-ratio test.  Also "null" (delta, vg, ve, ll), "lambda_gc", "n_used", "indxNA" and with map= "names".  backend: an
    am.SpectralBackend; one that AM() already ran on these genotypes is reused, nothing is rebuilt."""
    from . import am
    return am.GWAS(trait, X, geno, exact=exact, method=method, p_exact=p_exact, map=map, backend=backend, availmemGb=availmemGb,
                   device=device, Zmat=Zmat)


def GLMM(geno, status, X=None, tau=None, spa_cutoff=2.0, tol=1e-10, max_iter=50, map=None, backend=None, availmemGb=8, device=0):
    """Case/control association of every marker under the logistic mixed model, logit P(case) = x' alpha + b, b ~ N(0, tau K), with
    saddlepoint p-values (glmm.GLMM: GMMAT's score test and SAIGE's SPA; include/eagle_hip.h section 1d'''): what Logistic cannot do,
    take a kinship term, and what GWAS on a 0 / 1 trait does not do, respect the trait's distribution.  status as Logistic takes it
    (1 / 0 / NaN); X: (n, c <= 15) covariates WITH the intercept column, None = intercept only; tau= fixes the variance component
    (0.0: no kinship term).  Returns "score", "p_norm", "p_spa", "p", "spa_used", "beta", "se", "code", "evaluations" per marker, "null"
    (tau, alpha, converged, iterations), "lambda_gc", "n_used", "indxNA" and with map= "names"."""
    from . import glmm
    return glmm.GLMM(geno, status, X=X, tau=tau, spa_cutoff=spa_cutoff, tol=tol, max_iter=max_iter, map=map, backend=backend,
                     availmemGb=availmemGb, device=device)


# ---------------------------------------------------------------------------------------------------------------------------
# Tests of marker sets under the mixed model: burden and SKAT (include/eagle_hip.h section 1d''; device: rcpp_api.spectral_settest,
# am.SetTest).
# ---------------------------------------------------------------------------------------------------------------------------
SETTEST_MAX_MARKERS = 64


def settest_host(lam, UtX, Uty, Zrows, varE, varG, sets, omega=None):
    """rcpp_api.spectral_settest restated in numpy, set by set, by the rule of include/eagle_hip.h section 1d'': lam (n) the
    eigenvalues of K, UtX = U^T X (n x c, the intercept column included), Uty = U^T y, Zrows (L x n): row j = U^T m_j (what
    spectral_rows returns, transposed), the null model's varE and varG; sets, omega: as rcpp_api.settest_csr takes them ->
    {"stat" (k, 7) = Q, Ub, Vb, c_1 .. c_4; "info" (k, 2) = code, markers used; "score": k arrays s; "cov": k arrays Phi}.
    ValueError when G_xx fails its pivot rule (X^T H^-1 X is not positive definite).  Not bit-equal to the device (the order of the sums
    differs); tests/settest_truth.py holds both to 40-digit values."""
    lam = np.asarray(lam, dtype=np.float64).ravel()
    n = lam.size
    Ut = np.asarray(UtX, dtype=np.float64).reshape(n, -1)
    ut = np.asarray(Uty, dtype=np.float64).ravel()
    Zr = np.asarray(Zrows, dtype=np.float64).reshape(-1, n)
    c = Ut.shape[1]
    if not 1 <= c <= 14 or ut.size != n or n <= c + 1:
        raise ValueError("settest_host: UtX must be (n, c) with 1 <= c <= 14 and n > c + 1, Uty of length n")
    ptr, idx, w = rcpp_api.settest_csr(sets, omega)
    m_all = np.diff(ptr)
    if m_all.size and (m_all.min() < 1 or m_all.max() > SETTEST_MAX_MARKERS):
        raise ValueError("settest_host: every set must hold 1 to %d markers" % SETTEST_MAX_MARKERS)
    if idx.size and (idx.min() < 0 or idx.max() >= Zr.shape[0]):
        raise ValueError("settest_host: marker index out of range")
    if not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
        raise ValueError("settest_host: the weights must be finite and >= 0")
    h = varE + varG * lam
    if not np.all((h > 0.0) & np.isfinite(h)):
        raise ValueError("settest_host: varE + varG * lambda_k must be positive and finite")
    d = 1.0 / h
    vg2 = varG * varG
    k = m_all.size
    stat, info, score, cov = np.full((k, 7), np.nan), np.zeros((k, 2), dtype=np.int32), [], []
    for o in range(k):
        j, om = idx[ptr[o]:ptr[o + 1]], w[ptr[o]:ptr[o + 1]]
        m = j.size
        A = np.column_stack([Zr[j].T, Ut, ut])
        G = A.T @ (d[:, None] * A)
        G = np.tril(G) + np.tril(G, -1).T
        Lm = _logit_chol(G[m:m + c, m:m + c])                                         # the pivot rule, LMM_PIVOT_REL = 2^-40
        if Lm is None:
            raise ValueError("settest_host: X^T H^-1 X is not positive definite (collinear fixed effects)")
        B = _logit_solve(Lm, G[m:m + c, np.r_[0:m, m + c]])
        s = varG * (G[:m, m + c] - G[:m, m:m + c] @ B[:, m])
        Phi = np.tril(vg2 * (G[:m, :m] - G[:m, m:m + c] @ B[:, :m]))
        Phi = Phi + np.tril(Phi, -1).T                                                # the mirror is a copy of the lower triangle
        deg = ~(np.diag(Phi) > LMM_PIVOT_REL * vg2 * np.diag(G)[:m])
        s[deg] = 0.0
        Phi[deg, :] = 0.0
        Phi[:, deg] = 0.0
        Aw = Phi * np.outer(om, om)
        Aw2 = Aw @ Aw
        t = om * s
        st = (t @ t, t.sum(), Aw.sum(), np.trace(Aw), np.sum(Aw * Aw), np.sum(Aw * Aw2), np.sum(Aw2 * Aw2))
        none = not (st[2] > 0.0) or not (st[4] > 0.0)
        if not none:
            stat[o] = st
        info[o] = (2 if none else 0, m - int(deg.sum()))
        score.append(s)
        cov.append(Phi)
    return {"stat": stat, "info": info, "score": score, "cov": cov}


def _skat_traces(eig):
    lam = np.asarray(eig, dtype=np.float64).ravel()
    return tuple(float(np.sum(lam ** r)) for r in (1, 2, 3, 4))


def _skat_liu(Q, c):
    """P(sum_i lambda_i chi^2_1,i > Q) from c_r = sum_i lambda_i^r, r = 1 .. 4, by the moment matching of Liu, Tang & Zhang (2009) in
    the modified form that matches the kurtosis (SKAT's liu.mod)."""
    from scipy.special import chdtrc
    from scipy.stats import ncx2
    c1, c2, c3, c4 = (float(v) for v in c)
    if not (c2 > 0.0) or not all(math.isfinite(v) for v in (Q, c1, c2, c3, c4)):
        return float("nan")
    s1, s2 = c3 / c2 ** 1.5, c4 / (c2 * c2)
    # s1^2 >= s2 always (Cauchy-Schwarz), with equality for equal eigenvalues: a difference within 2^-40 s2 is the traces' rounding
    if s1 * s1 - s2 > LMM_PIVOT_REL * s2:
        a = 1.0 / (s1 - math.sqrt(s1 * s1 - s2))
        delta = s1 * a ** 3 - a * a
        l = a * a - 2.0 * delta
    else:
        l = 1.0 / s2
        a, delta = math.sqrt(l), 0.0
    q = (Q - c1) / math.sqrt(2.0 * c2) * math.sqrt(2.0) * a + l + delta
    if q <= 0.0:
        return 1.0
    return float(chdtrc(l, q) if delta == 0.0 else ncx2.sf(q, l, delta))


def _skat_saddle(Q, eig):
    """The same tail by Kuonen's (1999) saddlepoint approximation: K(t) = -1/2 sum log(1 - 2 t lambda_i), the root of K'(t) = Q by
    brentq, then Lugannani & Rice's formula.  NaN where the formula is singular (Q within 1e-6 of the mean in units of the sd)."""
    from scipy.optimize import brentq
    from scipy.special import ndtr
    lam = np.asarray(eig, dtype=np.float64).ravel()
    lam = lam[lam > 0.0]
    if lam.size == 0 or not math.isfinite(Q):
        return float("nan")
    lmax, mean, sd = float(lam.max()), float(lam.sum()), math.sqrt(2.0 * float(np.sum(lam * lam)))
    if Q <= 0.0:
        return 1.0
    if abs(Q - mean) <= 1e-6 * sd:
        return float("nan")
    lam = lam / lmax                                                                  # K' in units of lambda_max
    q = Q / lmax
    kp = lambda t: float(np.sum(lam / (1.0 - 2.0 * t * lam))) - q
    if Q > mean:
        lo, hi = 0.0, 0.5 * (1.0 - 0.5 / q)                                           # K'(hi) >= 1 / (1 - 2 hi) = 2 q
    else:
        lo, hi = -1.0, 0.0
        while kp(lo) > 0.0:
            lo *= 2.0
    t = brentq(kp, lo, hi, xtol=1e-300, rtol=8.9e-16, maxiter=500)
    K = -0.5 * float(np.sum(np.log1p(-2.0 * t * lam)))
    K2 = 2.0 * float(np.sum((lam / (1.0 - 2.0 * t * lam)) ** 2))
    w = math.copysign(math.sqrt(max(2.0 * (t * q - K), 0.0)), t)
    v = t * math.sqrt(K2)
    if w == 0.0 or v == 0.0:
        return float("nan")
    p = float(ndtr(-w)) + math.exp(-0.5 * w * w) / math.sqrt(2.0 * math.pi) * (1.0 / v - 1.0 / w)
    return min(max(p, 0.0), 1.0)


def skat_pvalue(Q, c=None, eig=None, method="liu"):
    """P(sum_i lambda_i chi^2_1,i > Q), the null distribution of SKAT's Q with lambda = the eigenvalues of Aw = W Phi W.
    method="liu": from the traces c = (c_1, c_2, c_3, c_4) = tr(Aw^r) -- what the device returns -- or from eig, by the modified moment
    matching of Liu et al. (2009): cheap, good to a few per cent down to p ~ 1e-4, drifting below.  method="saddle": from eig by
    Kuonen's saddlepoint approximation (Lugannani-Rice), whose RELATIVE error stays bounded in the far tail; NaN within 1e-6 standard
    deviations of the mean, where the formula is singular (use "liu" there)."""
    if method not in ("liu", "saddle"):
        raise ValueError("skat_pvalue: method must be \"liu\" or \"saddle\"")
    if method == "saddle":
        if eig is None:
            raise ValueError("skat_pvalue: the saddlepoint approximation needs eig=, the eigenvalues of W Phi W")
        return _skat_saddle(float(Q), eig)
    if c is None and eig is None:
        raise ValueError("skat_pvalue: give c=(c_1, c_2, c_3, c_4) or eig=")
    if c is None:
        lam = np.asarray(eig, dtype=np.float64).ravel()
        c = _skat_traces(lam[lam > 0.0])
    if len(c) != 4:
        raise ValueError("skat_pvalue: c holds the four traces c_1 .. c_4")
    return _skat_liu(float(Q), c)


def _set_map(who, map):
    if not hasattr(map, "keys") or "Chr" not in map or "Pos" not in map:
        raise ValueError("%s needs a map with Chr and Pos entries (ReadBim's)" % who)
    chrom, pos = [str(v) for v in map["Chr"]], np.asarray(map["Pos"], dtype=np.int64).ravel()
    if len(chrom) != pos.size:
        raise ValueError("%s: the map's Chr and Pos differ in length" % who)
    return chrom, pos


def _chrom_runs(chrom):
    """[(name, first, end)] of the runs of equal chromosome names, in file order."""
    runs, first = [], 0
    for j in range(1, len(chrom) + 1):
        if j == len(chrom) or chrom[j] != chrom[first]:
            runs.append((chrom[first], first, j))
            first = j
    return runs


def sets_from_windows(L_or_map, size=None, step=None, kb=None):
    """Windows of neighbouring markers as sets -> {"sets": list of int64 arrays of 0-based markers, "names": list of str}.
    L_or_map: the number of markers (one run) or a map (ReadBim's dict with Chr and Pos): windows are then cut at chromosome ends.
    size=: windows of `size` <= 64 markers, a new one every `step` markers (default: size, no overlap); the last window of a
    chromosome may be shorter.  kb= (needs a map with positions ascending inside a chromosome): windows of kb kilobases starting at the
    chromosome's first marker, a new one every `step` kilobases (default: kb); windows without a marker are left out, a window above
    64 markers is an error that names it."""
    if (size is None) == (kb is None):
        raise ValueError("sets_from_windows: give size= (markers) or kb= (kilobases), not both")
    if hasattr(L_or_map, "keys"):
        chrom, pos = _set_map("sets_from_windows", L_or_map)
        runs = _chrom_runs(chrom)
    else:
        if kb is not None:
            raise ValueError("sets_from_windows: kb= needs a map")
        runs, pos = [("", 0, int(L_or_map))], None
    sets, names = [], []
    if size is not None:
        size = int(size)
        step = size if step is None else int(step)
        if not 1 <= size <= SETTEST_MAX_MARKERS or step < 1:
            raise ValueError("sets_from_windows: 1 <= size <= %d and step >= 1" % SETTEST_MAX_MARKERS)
        for name, a, b in runs:
            for f in range(a, b, step):
                e = min(f + size, b)
                sets.append(np.arange(f, e, dtype=np.int64))
                names.append("%s%d-%d" % (name + ":" if name else "", f, e - 1))
                if e == b:
                    break
        return {"sets": sets, "names": names}
    width = int(round(float(kb) * 1000.0))
    stride = width if step is None else int(round(float(step) * 1000.0))
    if width < 1 or stride < 1:
        raise ValueError("sets_from_windows: kb and step must be positive")
    big = []
    for name, a, b in runs:
        p = pos[a:b]
        if np.any(np.diff(p) < 0):
            raise ValueError("sets_from_windows: positions must ascend inside chromosome %s" % name)
        start = int(p[0])
        while start <= int(p[-1]):
            f, e = a + int(np.searchsorted(p, start, "left")), a + int(np.searchsorted(p, start + width, "left"))
            if e > f:
                label = "%s:%d-%d" % (name, start, start + width - 1)
                if e - f > SETTEST_MAX_MARKERS:
                    big.append(label)
                sets.append(np.arange(f, e, dtype=np.int64))
                names.append(label)
            start += stride
    if big:
        raise ValueError("sets_from_windows: windows above %d markers: %s" % (SETTEST_MAX_MARKERS, ", ".join(big)))
    return {"sets": sets, "names": names}


def sets_from_table(map, regions):
    """Named regions (genes, candidate intervals) as sets -> {"sets", "names", "empty": names of regions that hold no marker, left
    out}.  map: ReadBim's dict; regions: rows (name, chr, start, end) or a mapping name -> (chr, start, end), positions in base pairs,
    both ends included.  Regions above 64 markers raise ValueError with their names."""
    chrom, pos = _set_map("sets_from_table", map)
    chrom = np.asarray(chrom)
    rows = [(k,) + tuple(v) for k, v in regions.items()] if hasattr(regions, "keys") else [tuple(r) for r in regions]
    sets, names, empty, big = [], [], [], []
    for r in rows:
        if len(r) != 4:
            raise ValueError("sets_from_table: a region is (name, chr, start, end)")
        name, ch, a, b = str(r[0]), str(r[1]), int(r[2]), int(r[3])
        j = np.flatnonzero((chrom == ch) & (pos >= a) & (pos <= b)).astype(np.int64)
        if j.size == 0:
            empty.append(name)
            continue
        if j.size > SETTEST_MAX_MARKERS:
            big.append("%s (%d)" % (name, j.size))
        sets.append(j)
        names.append(name)
    if big:
        raise ValueError("sets_from_table: regions above %d markers: %s" % (SETTEST_MAX_MARKERS, ", ".join(big)))
    return {"sets": sets, "names": names, "empty": empty}


def SetTest(trait, X, geno, sets, weights="equal", p_refine=1e-3, backend=None, map=None, availmemGb=8, device=0, Zmat=None):
    """Burden and SKAT tests of marker sets -- genes, windows, candidate regions -- under y = X beta + g + e with the null REML fit's
    variance components and the kinship AM() uses (am.SetTest; the EMMAX-SKAT / famSKAT tests): per set "n_markers", "n_used",
    "burden", "p_burden", "beta_burden", "Q", "p_skat", "p_skat_liu", "refined", "code", plus "null", "names", "n_used_individuals",
    "indxNA".  sets: a list of arrays of 0-based markers or what sets_from_windows / sets_from_table return; weights: "equal",
    ("beta", a, b) (Beta(MAF; a, b), default (1, 25)) or one weight per marker.  The sets with a Liu p-value below p_refine get the
    saddlepoint p-value from the eigenvalues of W Phi W.  backend: an am.SpectralBackend; one that AM() or GWAS() already ran on these
    genotypes is reused, nothing is rebuilt."""
    from . import am
    return am.SetTest(trait, X, geno, sets, weights=weights, p_refine=p_refine, backend=backend, map=map, availmemGb=availmemGb,
                      device=device, Zmat=Zmat)


# ---- pairwise haplotype EM, D' and haplotype blocks (include/eagle_hip.h section 1b''''vii): the restatement in numpy and the interface ----
def hap_ld_cells(n, si, qi, sj, qj, d, e, f, h):
    """The nine cells of the 3 x 3 genotype table of a pair of markers from its integer sums (rule 2 of section 1b''''vii) -> dict of
    int64 arrays "N00" .. "N22" (first digit: the number of B alleles at marker i); N11 is x, the double heterozygotes."""
    si, qi, sj, qj, d, e, f, h = (np.asarray(a, dtype=np.int64) for a in (si, qi, sj, qj, d, e, f, h))
    return {"N22": (e + f + h + d) // 4, "N00": (e - f - h + d) // 4, "N20": (e - f + h - d) // 4, "N02": (e + f - h - d) // 4,
            "N12": (qj + sj - e - f) // 2, "N10": (qj - sj - e + f) // 2, "N21": (qi + si - e - h) // 2, "N01": (qi - si - e + h) // 2,
            "N11": int(n) - qi - qj + e}


def hap_ld_pairs_host(n, si, qi, sj, qj, d, e, f, h, tol=1e-10, max_iter=1000):
    """Rules 3 to 5 of section 1b''''vii for arrays of pairs of POLYMORPHIC markers, vectorised over the pairs with a per-pair stop
    mask and the device's order of elementwise fp64 operations -> {"p": fp64 (4, pairs) = pBB, pBA, pAB, pAA, "dprime", "r2", "pmin":
    fp64, "code": int32 (0 converged, 1 stopped at max_iter), "iterations": int32}."""
    c = hap_ld_cells(n, si, qi, sj, qj, d, e, f, h)
    si, sj = np.asarray(si, dtype=np.int64), np.asarray(sj, dtype=np.int64)
    kBB = (2 * c["N22"] + c["N21"] + c["N12"]).astype(np.float64)
    kBA = (2 * c["N20"] + c["N21"] + c["N10"]).astype(np.float64)
    kAB = (2 * c["N02"] + c["N01"] + c["N12"]).astype(np.float64)
    kAA = (2 * c["N00"] + c["N01"] + c["N10"]).astype(np.float64)
    x = c["N11"]
    n = int(n)
    T = np.float64(2 * n)
    bi, bj = n + si, n + sj
    pi, qi_ = bi.astype(np.float64) / T, (2 * n - bi).astype(np.float64) / T
    pj, qj_ = bj.astype(np.float64) / T, (2 * n - bj).astype(np.float64) / T
    pipj, piqj, qipj, qiqj = pi * pj, pi * qj_, qi_ * pj, qi_ * qj_
    zero = x == 0
    pBB, pBA, pAB, pAA = (np.where(zero, k / T, start) for k, start in ((kBB, pipj), (kBA, piqj), (kAB, qipj), (kAA, qiqj)))
    code, iters = np.zeros(x.shape, dtype=np.int32), np.zeros(x.shape, dtype=np.int32)
    live = np.flatnonzero(~zero)
    xd = x.astype(np.float64)
    it = 0
    while live.size:
        it += 1
        u, v = pBB[live] * pAA[live], pBA[live] * pAB[live]
        den = u + v
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(den > 0.0, u / den, 0.5)
        xt = xd[live] * t
        xo = xd[live] - xt
        nBB = (kBB[live] + xt) / T
        delta = np.abs(nBB - pBB[live])
        pBB[live], pAA[live], pBA[live], pAB[live] = nBB, (kAA[live] + xt) / T, (kBA[live] + xo) / T, (kAB[live] + xo) / T
        iters[live] = it
        done = delta <= tol
        if it == int(max_iter):
            code[live[~done]] = 1
            break
        live = live[~done]
    D = pBB - pipj
    dmax = np.where(D >= 0.0, np.minimum(piqj, qipj), np.minimum(pipj, qiqj))
    dprime = np.clip(D / dmax, -1.0, 1.0)
    r2 = (D * D) / ((pi * qi_) * (pj * qj_))
    pmin = np.minimum(np.minimum(pBB, pBA), np.minimum(pAB, pAA))
    return {"p": np.stack([pBB, pBA, pAB, pAA]), "dprime": dprime, "r2": r2, "pmin": pmin, "code": code, "iterations": iters}


def _hap_pack_bits(bits):
    """bool (L, window) -> uint64 (L, ceil(window / 64)), column o - 1 at bit (o - 1) % 64 of word (o - 1) // 64."""
    L, window = bits.shape
    wide = np.zeros((L, (window + 63) // 64 * 64), dtype=np.uint8)
    wide[:, :window] = bits
    return np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(L, -1)


def _hap_unpack_bits(mask, window):
    """uint64 (L, ceil(window / 64)) -> bool (L, window)."""
    m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint64)).astype("<u8")
    return np.unpackbits(m.view(np.uint8).reshape(m.shape[0], -1), axis=1, bitorder="little")[:, :int(window)].astype(bool)


def hap_ld_host(Mt8, window, tol=1e-10, max_iter=1000, fg_cut=0.01, dprime_cut=0.8):
    """rcpp_api.hap_ld restated in numpy: Mt8 = int8 (L, n) marker-major genotypes in {-1, 0, +1} (a missing call is a het) -> {"recomb",
    "strong": uint64 (L, ceil(window / 64)), "dprime", "r2": fp64 (L, window), -2.0 / -1.0 for an undefined pair, "counts": int64 (4),
    and for the tests "pmin", "pBB": fp64, "iterations", "code": int32 (L, window), 0 where undefined}.  The rule of include/eagle_hip.h
    section 1b''''vii with the same order of elementwise operations: the same words as the device."""
    G = np.asarray(Mt8)
    L, n = G.shape
    window = int(window)
    if not 1 <= window <= 256:
        raise ValueError("hap_ld_host: 1 <= window <= 256")
    F = G.astype(np.float64)                                   # products and sums of small integers: exact in fp64 below 2^53
    F2 = F * F
    Gi = G.astype(np.int64)
    s, q = Gi.sum(axis=1), (Gi * Gi).sum(axis=1)
    b = n + s
    poly = (b > 0) & (b < 2 * n) & (n >= 2)
    dprime, r2 = np.full((L, window), -2.0), np.full((L, window), -1.0)
    pmin, pBB = np.zeros((L, window)), np.zeros((L, window))
    iters, code = np.zeros((L, window), dtype=np.int32), np.zeros((L, window), dtype=np.int32)
    defined = np.zeros((L, window), dtype=bool)
    batch, held = [], 0                                        # offsets are run together: the slowest pair of a batch sets its trip count

    def run():
        i, o = np.concatenate([b[0] for b in batch]), np.concatenate([b[1] for b in batch])
        sums = [np.concatenate([b[2][k] for b in batch]) for k in range(4)]
        res = hap_ld_pairs_host(n, s[i], q[i], s[i + o], q[i + o], sums[0], sums[1], sums[2], sums[3], tol, max_iter)
        defined[i, o - 1] = True
        dprime[i, o - 1], r2[i, o - 1], pmin[i, o - 1], pBB[i, o - 1] = res["dprime"], res["r2"], res["pmin"], res["p"][0]
        iters[i, o - 1], code[i, o - 1] = res["iterations"], res["code"]

    for o in range(1, min(window, L - 1) + 1):
        ok = np.flatnonzero(poly[:-o] & poly[o:])              # markers i with j = i + o, both polymorphic
        if not ok.size:
            continue
        A, B, A2, B2 = F[ok], F[ok + o], F2[ok], F2[ok + o]
        batch.append((ok, np.full(ok.size, o), [np.rint(np.einsum("ij,ij->i", a, c)).astype(np.int64) for a, c in ((A, B), (A2, B2), (A2, B), (A, B2))]))
        held += ok.size
        if held >= 1 << 18:
            run()
            batch, held = [], 0
    if batch:
        run()
    rec = defined & (pmin > fg_cut)
    strong = defined & (np.abs(dprime) >= dprime_cut)
    counts = np.array([defined.sum(), code.sum(), rec.sum(), strong.sum()], dtype=np.int64)
    return {"recomb": _hap_pack_bits(rec), "strong": _hap_pack_bits(strong), "dprime": dprime, "r2": r2, "counts": counts, "pmin": pmin,
            "pBB": pBB, "iterations": iters, "code": code}


def _hap_reach(L, chrom, pos, kb):
    """same(i, j) for i <= j: marker j may share a block that starts at i -- the same chromosome, and within kb of marker i when given."""
    span = None if kb is None else int(round(float(kb) * 1000.0))
    if span is not None and (pos is None or span < 1):
        raise ValueError("hap_blocks_host: kb needs positions and must be at least 0.001")

    def same(i, j):
        if chrom is not None and chrom[j] != chrom[i]:
            return False
        return span is None or abs(int(pos[j]) - int(pos[i])) <= span
    return same


def hap_blocks_host(recomb, strong, window, chrom=None, pos=None, kb=None, method="fourgamete", min_snp=2):
    """The partition of the map into haplotype blocks from the two verdict masks of hap_ld (uint64 (L, ceil(window / 64))), greedy in
    map order -> (first int64 (B), last int64 (B), block_of int64 (L), -1 outside any reported block).
    "fourgamete": the block [i, j] grows to j + 1 while j + 1 - i <= window, marker j + 1 lies on the chromosome of i (chrom: one label
    per marker) and within kb kilobases of it (pos: base pairs), and no pair (k, j + 1), i <= k <= j, is RECOMBINANT; an undefined pair
    does not object, so a monomorphic marker joins.  "spine" (Haploview's solid spine of LD): from i the largest j in reach with
    STRONG(i, k) for every i < k <= j and STRONG(k, j) for every i <= k < j.  Either way the next block starts at j + 1, and blocks below
    min_snp markers are not reported."""
    window, min_snp = int(window), int(min_snp)
    if method not in ("fourgamete", "spine"):
        raise ValueError("hap_blocks_host: method is 'fourgamete' or 'spine'")
    if not 1 <= window <= 256 or min_snp < 1:
        raise ValueError("hap_blocks_host: 1 <= window <= 256 and min_snp >= 1")
    bits = _hap_unpack_bits(recomb if method == "fourgamete" else strong, window)       # bits[k, j - k - 1]: the pair (k, j)
    L = bits.shape[0]
    chrom = None if chrom is None else np.asarray(chrom)
    pos = None if pos is None else np.asarray(pos, dtype=np.int64)
    same = _hap_reach(L, chrom, pos, kb)
    first, last = [], []
    block_of = np.full(L, -1, dtype=np.int64)
    i = 0
    while i < L:
        j = i
        if method == "fourgamete":
            while j + 1 < L and j + 1 - i <= window and same(i, j + 1):
                k = np.arange(i, j + 1)
                if bits[k, j - k].any():
                    break
                j += 1
        else:
            reach = i
            while reach + 1 < L and reach + 1 - i <= window and same(i, reach + 1) and bits[i, reach - i]:
                reach += 1
            for cand in range(reach, i, -1):
                k = np.arange(i, cand)
                if bits[k, cand - k - 1].all():
                    j = cand
                    break
        if j - i + 1 >= min_snp:
            block_of[i:j + 1] = len(first)
            first.append(i)
            last.append(j)
        i = j + 1
    return np.asarray(first, dtype=np.int64), np.asarray(last, dtype=np.int64), block_of


def _hap_source(who, geno, map, kb):
    """(n, L, map or None, chrom labels or None, pos int64 or None) of a HapLD / HapBlocks call."""
    n, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    errs = []
    map = _ld_map(who, map, geno, L, errs.append)
    if map is False:
        raise ValueError(who + ":" + errs[0])
    if map is None:
        if kb is not None:
            raise ValueError("%s: kb= needs a map with Chr and Pos entries" % who)
        return n, L, None, None, None
    chrom = np.asarray([str(c) for c in map["Chr"]])
    pos = np.asarray(map["Pos"]).ravel()
    if not np.array_equal(pos.astype(np.int64), pos):
        raise ValueError("%s: the map's positions must be whole numbers of base pairs" % who)
    if kb is not None and int(round(float(kb) * 1000.0)) < 1:
        raise ValueError("%s: kb must be at least 0.001" % who)
    return n, L, map, chrom, pos.astype(np.int64)


def HapLD(geno, window=50, map=None, kb=None, tol=1e-10, max_iter=1000, availmemGb=8, device=0):
    """Lewontin's D' and the haplotype r2 of every pair of markers at most `window` <= 256 apart, from haplotype frequencies estimated
    by EM on the unphased genotypes (include/eagle_hip.h section 1b''''vii; rcpp_api.hap_ld) -> {"dprime": fp64 (L, window), signed,
    entry (i, o - 1) = the pair (i, i + o), NaN where the pair is not defined, "r2": likewise, "defined": bool (L, window), "counts":
    int64 (4) of rcpp_api.hap_ld, "mean_abs_dprime": fp64 (window), the mean |D'| of the defined pairs per offset, NaN without one}.  A
    pair is not defined beyond the panel's end or with a monomorphic member; with a map (ReadBim's dict) also across chromosomes, and
    with kb= more than kb kilobases apart.  The EM starts at equilibrium (Haploview's); it is not PLINK's cubic solver."""
    n, L, map, chrom, pos = _hap_source("HapLD", geno, map, kb)
    window = int(window)
    raw = rcpp_api.hap_ld(geno["asciifileMt"], (n, L), window, tol, max_iter, bands=True, masks=False, availmemGb=availmemGb, device=device)
    defined = raw["r2"] >= 0.0
    if chrom is not None:
        span = None if kb is None else int(round(float(kb) * 1000.0))
        for o in range(1, min(window, L - 1) + 1):
            ok = chrom[:-o] == chrom[o:]
            if span is not None:
                ok &= np.abs(pos[o:] - pos[:-o]) <= span
            defined[:L - o, o - 1] &= ok
    dprime, r2 = np.where(defined, raw["dprime"], np.nan), np.where(defined, raw["r2"], np.nan)
    cnt = defined.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(cnt > 0, np.where(defined, np.abs(raw["dprime"]), 0.0).sum(axis=0) / cnt, np.nan)
    return {"dprime": dprime, "r2": r2, "defined": defined, "counts": raw["counts"], "mean_abs_dprime": mean}


def HapBlocks(geno, method="fourgamete", window=50, map=None, kb=None, min_snp=2, fg_cut=0.01, dprime=0.8, tol=1e-10, max_iter=1000,
              availmemGb=8, device=0):
    """The haplotype blocks of a panel -> {"blocks": {"first", "last": int64 (B), 0-based markers, both ends included, "n_markers": int64,
    "chrom": list of str ("" without a map), "start", "end": int64 (the markers' positions; the marker indices without a map),
    "length": int64 = end - start + 1}, "block_of": int64 (L), the block of every marker, -1 outside any, "share": the share of markers
    in blocks, "counts": int64 (4) of rcpp_api.hap_ld, "method", "window"}.  The pairwise verdicts come from the device (rcpp_api.hap_ld:
    RECOMBINANT iff the smallest EM haplotype frequency is above fg_cut, STRONG iff |D'| >= dprime; include/eagle_hip.h section
    1b''''vii), the partition is hap_blocks_host's: method "fourgamete" (Wang et al. 2002, PLINK's and Haploview's four-gamete rule) or
    "spine" (Haploview's solid spine of LD), greedy in map order, cut at chromosome ends with a map (ReadBim's dict) and at kb kilobases
    from the block's first marker with kb=.  Blocks below min_snp markers are not reported.  Gabriel's confidence-interval blocks are
    out of scope.  sets_from_blocks turns the result into sets for SetTest."""
    n, L, map, chrom, pos = _hap_source("HapBlocks", geno, map, kb)
    window = int(window)
    raw = rcpp_api.hap_ld(geno["asciifileMt"], (n, L), window, tol, max_iter, fg_cut, dprime, availmemGb=availmemGb, device=device)
    first, last, block_of = hap_blocks_host(raw["recomb"], raw["strong"], window, chrom, pos, kb, method, min_snp)
    at = np.arange(L, dtype=np.int64) if pos is None else pos
    start, end = at[first], at[last]
    blocks = {"first": first, "last": last, "n_markers": last - first + 1, "chrom": ["" if chrom is None else str(chrom[f]) for f in first],
              "start": start, "end": end, "length": np.abs(end - start) + 1}
    return {"blocks": blocks, "block_of": block_of, "share": float((block_of >= 0).mean()) if L else 0.0, "counts": raw["counts"],
            "method": method, "window": window}


def sets_from_blocks(blocks, max_markers=64, names=None):
    """Haplotype blocks as sets -> {"sets": list of int64 arrays of 0-based markers, "names": list of str}, as sets_from_windows
    returns them.  blocks: what HapBlocks returns, or its "blocks" table.  A block above max_markers <= 64 markers (SetTest's limit) is
    cut into consecutive pieces of at most max_markers markers, named name/1, name/2, ...  names: one name per block; default
    "chrom:first-last" ("first-last" without a chromosome)."""
    tab = blocks["blocks"] if hasattr(blocks, "keys") and "blocks" in blocks else blocks
    max_markers = int(max_markers)
    if not 1 <= max_markers <= SETTEST_MAX_MARKERS:
        raise ValueError("sets_from_blocks: 1 <= max_markers <= %d" % SETTEST_MAX_MARKERS)
    first, last = np.asarray(tab["first"], dtype=np.int64).ravel(), np.asarray(tab["last"], dtype=np.int64).ravel()
    chrom = list(tab["chrom"]) if "chrom" in tab else [""] * first.size
    if first.size != last.size or len(chrom) != first.size or np.any(last < first) or np.any(first < 0):
        raise ValueError("sets_from_blocks: a block is first <= last, both 0-based markers")
    if names is not None and len(names) != first.size:
        raise ValueError("sets_from_blocks: names must hold one name per block (%d)" % first.size)
    sets, out = [], []
    for b in range(first.size):
        f, e = int(first[b]), int(last[b]) + 1
        name = str(names[b]) if names is not None else "%s%d-%d" % (str(chrom[b]) + ":" if str(chrom[b]) else "", f, e - 1)
        pieces = range(f, e, max_markers)
        for k, a in enumerate(pieces):
            sets.append(np.arange(a, min(a + max_markers, e), dtype=np.int64))
            out.append(name if len(pieces) == 1 else "%s/%d" % (name, k + 1))
    return {"sets": sets, "names": out}

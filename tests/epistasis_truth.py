"""Truth for the epistasis tests: plain Python loops over the individuals and exact rational arithmetic (fractions.Fraction).  It shares no
code with the feature and no numpy: the eleven sums of include/eagle_hip.h section 1b''''ii, Delta, Sxx, Sxy, Syy and the exact
F = (n - 4) Sxy^2 / (Sxx Syy - Sxy^2)."""
from fractions import Fraction


def sums(gi, gj, y):
    """The sums of one pair -> dict of Python ints.  gi, gj, y: sequences of ints of one length."""
    gi, gj, y = [int(v) for v in gi], [int(v) for v in gj], [int(v) for v in y]
    n = len(y)
    assert len(gi) == n and len(gj) == n
    out = dict(n=n, Y=0, T=0, si=0, qi=0, ui=0, sj=0, qj=0, uj=0, d=0, e=0, f=0, h=0, z=0)
    for a, b, v in zip(gi, gj, y):
        out["Y"] += v
        out["T"] += v * v
        out["si"] += a
        out["qi"] += a * a
        out["ui"] += v * a
        out["sj"] += b
        out["qj"] += b * b
        out["uj"] += v * b
        out["d"] += a * b
        out["e"] += a * a * b
        out["f"] += a * b * b
        out["h"] += a * a * b * b
        out["z"] += v * a * b
    return out


def det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def adj3(m):
    """The adjugate: adj[r][c] = cofactor(c, r)."""
    def minor(r, c):
        rows = [x for x in range(3) if x != r]
        cols = [x for x in range(3) if x != c]
        return m[rows[0]][cols[0]] * m[rows[1]][cols[1]] - m[rows[0]][cols[1]] * m[rows[1]][cols[0]]
    return [[(-1) ** (r + c) * minor(c, r) for c in range(3)] for r in range(3)]


def quad(A, v, w):
    return sum(v[r] * A[r][c] * w[c] for r in range(3) for c in range(3))


def S(t):
    """(Delta, Sxx, Sxy, Syy) from sums(): Python ints."""
    B = [[t["n"], t["si"], t["sj"]], [t["si"], t["qi"], t["d"]], [t["sj"], t["d"], t["qj"]]]
    Delta, A = det3(B), adj3(B)
    c, u = (t["d"], t["e"], t["f"]), (t["Y"], t["ui"], t["uj"])
    return Delta, Delta * t["h"] - quad(A, c, c), Delta * t["z"] - quad(A, c, u), Delta * t["T"] - quad(A, u, u)


def defined(t):
    Delta, Sxx, _, _ = S(t)
    return t["n"] > 4 and Delta > 0 and Sxx > 0


def exact_F(t):
    """None where the pair is undefined, "inf" where Sxx Syy = Sxy^2 (r2 = 1, or Syy = 0), else the exact Fraction."""
    if not defined(t):
        return None
    _, Sxx, Sxy, Syy = S(t)
    den = Sxx * Syy - Sxy * Sxy
    assert den >= 0                                             # Cauchy-Schwarz on exact sums
    if den == 0:
        return "inf"
    return Fraction((t["n"] - 4) * Sxy * Sxy, den)


def exact_r2(t):
    _, Sxx, Sxy, Syy = S(t)
    return Fraction(Sxy * Sxy, Sxx * Syy)


def pair_tested(i, j, chrom, gap):
    return not (j - i <= gap and (chrom is None or chrom[i] == chrom[j]))

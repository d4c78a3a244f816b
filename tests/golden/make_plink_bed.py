"""Writes tests/golden/plink_150x100.{bed,bim,fam}: the genotypes of geno_150x100.txt (150 individuals x 100 markers, digits 0/1/2)
as a PLINK binary fileset in SNP-major mode, digit 0 -> 00 (homozygous A1), 1 -> 10 (heterozygous), 2 -> 11 (homozygous A2), none
missing.  Written here byte by byte, without the package, so that the fixture does not depend on the code it tests.

    python tests/golden/make_plink_bed.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    g = np.loadtxt(os.path.join(HERE, "geno_150x100.txt"), dtype=np.int64)   # individuals x markers
    n, L = g.shape
    code = np.array([0b00, 0b10, 0b11])[g.T]                                  # markers x individuals
    rows = bytearray(b"\x6c\x1b\x01")
    for j in range(L):
        for b in range((n + 3) // 4):
            byte = 0
            for q in range(4):
                if 4 * b + q < n:
                    byte |= int(code[j, 4 * b + q]) << (2 * q)
            rows.append(byte)
    prefix = os.path.join(HERE, "plink_150x100")
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes(rows))
    with open(prefix + ".bim", "w") as f:
        for j in range(L):
            f.write("%d\trs%04d\t0\t%d\tA\tB\n" % (1 + j // 25, 1001 + j, 10000 * (j + 1)))
    with open(prefix + ".fam", "w") as f:
        for i in range(n):
            f.write("F%d I%d 0 0 %d -9\n" % (i + 1, i + 1, 1 + i % 2))


if __name__ == "__main__":
    main()

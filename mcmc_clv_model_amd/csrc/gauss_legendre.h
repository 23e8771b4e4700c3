// The 16-point Gauss-Legendre rule on [-1, 1]: nodes x_j ascending and weights w_j, rounded once from
// 40 digits.  Written by tools/make_gauss_legendre.py; do not edit.  tests/test_mle_ext_cpu.py checks it
// against numpy's leggauss and the monomials up to degree 31.
#pragma once

#define CLV_GL_Q 16
#define CLV_GL_X_INIT { \
  -0x1.fa92c264d787ep-1, \
  -0x1.e39f56616f9b0p-1, \
  -0x1.bb3403514e483p-1, \
  -0x1.82c45dda4726bp-1, \
  -0x1.3c5a466d5e8b8p-1, \
  -0x1.d50259a43a772p-2, \
  -0x1.205cae642337cp-2, \
  -0x1.852bd6676a9f9p-4, \
  0x1.852bd6676a9f9p-4, \
  0x1.205cae642337cp-2, \
  0x1.d50259a43a772p-2, \
  0x1.3c5a466d5e8b8p-1, \
  0x1.82c45dda4726bp-1, \
  0x1.bb3403514e483p-1, \
  0x1.e39f56616f9b0p-1, \
  0x1.fa92c264d787ep-1, \
}
#define CLV_GL_W_INIT { \
  0x1.bcddab4b7c211p-6, \
  0x1.fdfb1a2c1265dp-5, \
  0x1.85c4ee79cc258p-4, \
  0x1.fe7af2bad386ap-4, \
  0x1.325f61bca3cbfp-3, \
  0x1.5a6ebbb5a75fcp-3, \
  0x1.75f8c77e0c00fp-3, \
  0x1.83feae80e4dfcp-3, \
  0x1.83feae80e4dfcp-3, \
  0x1.75f8c77e0c00fp-3, \
  0x1.5a6ebbb5a75fcp-3, \
  0x1.325f61bca3cbfp-3, \
  0x1.fe7af2bad386ap-4, \
  0x1.85c4ee79cc258p-4, \
  0x1.fdfb1a2c1265dp-5, \
  0x1.bcddab4b7c211p-6, \
}

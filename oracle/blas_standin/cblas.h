/* cblas.h -- TEST INFRASTRUCTURE.  A stand-in for the system BLAS header, so
 * that the reference's matrix.cc compiles where no BLAS is installed.  It
 * declares the one routine matrix.cc calls (cblas_sgemm, from MatMat) with the
 * public CBLAS argument order and the standard enum values; the definition is
 * in oracle/ref_harness.cc. */
#ifndef CATEARS_ORACLE_CBLAS_STANDIN_H_
#define CATEARS_ORACLE_CBLAS_STANDIN_H_

#ifdef __cplusplus
extern "C" {
#endif

enum CBLAS_ORDER { CblasRowMajor = 101, CblasColMajor = 102 };
enum CBLAS_TRANSPOSE { CblasNoTrans = 111, CblasTrans = 112, CblasConjTrans = 113 };

void cblas_sgemm(enum CBLAS_ORDER order, enum CBLAS_TRANSPOSE trans_a, enum CBLAS_TRANSPOSE trans_b,
                 int m, int n, int k, float alpha, const float *a, int lda, const float *b, int ldb,
                 float beta, float *c, int ldc);

#ifdef __cplusplus
}
#endif

#endif

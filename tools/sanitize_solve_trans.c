/*
 * sanitize_solve_trans.c -- AddressSanitizer + UBSan over the host sweep of the transposed solve (pg_sptrsv.cpp, pg_api.cpp), on the
 * CPU and in a program of its own: the checker's host code (-DPANGULU_AMD_TEST_HOOKS) is compiled WITH the sanitizers together with
 * this file, the operators come from the oracle's CPU library, no GPU is touched and nothing is preloaded.  From the repository root,
 * after a normal build (the HIP object and the oracle library exist):
 *
 *   cd pangulu_amd/csrc && g++ -I/opt/rocm/include -I../../include -I../../oracle -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined \
 *       -fno-omit-frame-pointer -DCALCULATE_TYPE_R64 -DPANGULU_AMD_TEST_HOOKS -x c++ host/pg_*.cpp ../../tools/sanitize_solve_trans.c \
 *       -x none build/r64/pg_hip_platform.o -o /tmp/sanitize_solve_trans -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lamdhip64 -ldl -lpthread
 *   ASAN_OPTIONS=detect_leaks=0 /tmp/sanitize_solve_trans $PWD/../../oracle/_build/libpangulu_oracle_r64.so
 *
 * A 3D convection-diffusion matrix (unsymmetric values), scaling off and on, nb = 16: A^T X = B for three right-hand sides with
 * ldb = n + 2, the residual checked, the slack rows checked, the return codes 2 and 3 exercised.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pangulu.h"
#include "pangulu_amd_ext.h"
#include "pangulu_amd_test_hooks.h"

int main(int argc, char **argv)
{
    if (argc < 2 || pangulu_amd_use_platform_library(argv[1], PANGULU_PLATFORM_CPU_NAIVE) != 0)
    {
        fprintf(stderr, "usage: sanitize_solve_trans <path of libpangulu_oracle_r64.so>\n");
        return 2;
    }
    const int nx = 6, n = nx * nx * nx, nrhs = 3, ldb = n + 2;
    sparse_pointer_t *cp = (sparse_pointer_t *)calloc(n + 1, sizeof *cp);
    sparse_index_t *ri = (sparse_index_t *)malloc(sizeof *ri * 7 * n);
    double *va = (double *)malloc(sizeof *va * 7 * n);
    sparse_pointer_t nnz = 0;
    for (int c = 0; c < n; c++) /* column c: the rows that have an entry in it, ascending */
    {
        const int x = c / (nx * nx), y = c / nx % nx, z = c % nx;
        const int nbr[7][2] = {{-nx * nx, x > 0}, {-nx, y > 0}, {-1, z > 0}, {0, 1}, {1, z < nx - 1}, {nx, y < nx - 1}, {nx * nx, x < nx - 1}};
        for (int k = 0; k < 7; k++)
            if (nbr[k][1])
            {
                ri[nnz] = (sparse_index_t)(c + nbr[k][0]);
                va[nnz] = k == 3 ? 7.3 : k == 6 ? -1.8 : -1.0 + 0.01 * (c % 5); /* entry (c + nx nx, c) carries the convection term */
                nnz++;
            }
        cp[c + 1] = nnz;
    }
    int bad = 0;
    for (int scaling = 0; scaling < 2; scaling++)
    {
        pangulu_amd_set_scaling(scaling);
        pangulu_init_options io;
        memset(&io, 0, sizeof io);
        io.nthread = 2, io.nb = 16, io.sizeof_value = (int)sizeof(double), io.mpi_recv_buffer_level = 0.5f;
        pangulu_gstrf_options fo;
        pangulu_gstrs_options so;
        memset(&fo, 0, sizeof fo), memset(&so, 0, sizeof so);
        void *h = NULL;
        pangulu_init((sparse_index_t)n, nnz, cp, ri, va, &io, &h);
        double *B = (double *)malloc(sizeof *B * ldb * nrhs), *X = (double *)malloc(sizeof *X * ldb * nrhs);
        for (int i = 0; i < ldb * nrhs; i++)
            B[i] = i % ldb < n ? sin(0.37 * i) : -777.25;
        memcpy(X, B, sizeof *X * ldb * nrhs);
        bad += pangulu_amd_gstrs_trans(X, nrhs, ldb, PANGULU_AMD_TRANS_T, &so, &h) != 1; /* not factorised yet */
        pangulu_gstrf(&fo, &h);
        bad += pangulu_amd_gstrs_trans(X, nrhs, n - 1, PANGULU_AMD_TRANS_T, &so, &h) != 2;
        bad += pangulu_amd_gstrs_trans(X, nrhs, ldb, 7, &so, &h) != 3;
        bad += memcmp(X, B, sizeof *X * ldb * nrhs) != 0;
        bad += pangulu_amd_gstrs_trans(X, nrhs, ldb, PANGULU_AMD_TRANS_T, &so, &h) != 0;
        double worst = 0;
        for (int j = 0; j < nrhs; j++)
        {
            double rr = 0, bb = 0;
            for (int c = 0; c < n; c++) /* (A^T x)[c] = column c of A . x */
            {
                double acc = 0;
                for (sparse_pointer_t p = cp[c]; p < cp[c + 1]; p++)
                    acc += va[p] * X[j * ldb + ri[p]];
                rr += (acc - B[j * ldb + c]) * (acc - B[j * ldb + c]), bb += B[j * ldb + c] * B[j * ldb + c];
            }
            worst = fmax(worst, sqrt(rr / bb));
            bad += X[j * ldb + n] != -777.25 || X[j * ldb + n + 1] != -777.25;
        }
        printf("scaling %d: worst || A^T x - b || / || b || = %.3e\n", scaling, worst);
        bad += !(worst < 1e-12);
        pangulu_finalize(&h);
        free(B), free(X);
    }
    free(cp), free(ri), free(va);
    printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad != 0;
}

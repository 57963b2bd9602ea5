// kkt_driver.hpp -- the drivers of the saddle-point operator K = [A B'; B -C], described where they
// are defined (kkt_driver.cpp).  Every d_* is device memory; the work goes to K's context stream.
#pragma once
#include <string>

#include "handles.hpp"

namespace cpk {

void kkt_assemble(cpk_kkt K);  // K's device copy and value map from its handles (n, m, ctx are set)
void kkt_apply(cpk_kkt K, const double *d_z, double *d_y);
void kkt_resid_block(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_B, int64_t ldb, double *d_R,
                     int64_t ldr, double *d_norms);
void kkt_resid_exact_block(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_B, int64_t ldb, double *d_R,
                           int64_t ldr, double *d_norms);
void kkt_solve_core(cpk_kkt K, int method, const double *d_b, cpk_pc M, const cpk_opts *opts, double *d_x, int warm,
                    cpk_stats *stats, double *res);
void kkt_refined_core(cpk_kkt K, int method, const double *d_b, cpk_pc M, const cpk_opts *opts, double *d_x, int warm,
                      int max_steps, cpk_stats *stats, double *res, int *steps_out, bool *wrote_x = nullptr);
void kkt_adjoint_core(cpk_kkt K, cpk_kkt KT, int method, const double *d_x, const double *d_gx, cpk_pc M, const cpk_opts *opts,
                      double *d_lam, int warm, double *d_gA, double *d_gB, double *d_gC, cpk_stats *stats, double *res);
int kkt_solve_multi_core(cpk_kkt K, int method, int64_t k, const double *d_B, int64_t ldb, cpk_pc M, const cpk_opts *opts,
                         double *d_X, int64_t ldx, int warm, cpk_stats *stats, int *col_status, double *res, std::string *msg);
void kkt_sample_core(cpk_kkt K, int64_t k, const double *d_X, int64_t ldx, const double *d_L, int64_t ldl, double *d_gA,
                     double *d_gB, double *d_gC);

}  // namespace cpk

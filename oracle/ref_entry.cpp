// TEST INFRASTRUCTURE ONLY.  extern "C" doors into the reference's own translation units, which oracle/Makefile (target
// `ref`) compiles unmodified, from where they lie, against the stand-in headers of oracle/refstub/.  This file is this
// project's own code: it declares the reference's entry points by their exported prototypes (E/src/RcppExports.cpp:9-143,
// E/src/createM_ASCII_rcpp.h), turns plain pointers into the stand-in types, catches Rcpp::stop and hands back what
// message() recorded.  Return codes: 0 ok, -1 Rcpp::stop (text in er_last_error), -2 the stand-in refused an access the
// reference leaves undefined (text in er_last_error).
#include <RcppEigen.h>

#include <string>
#include <vector>

Eigen::MatrixXd ReadBlock(std::string asciifname, long start_row, long numcols, long numrows_in_block);
std::vector<long> ReshapeM_rcpp(Rcpp::CharacterVector fnameM, Rcpp::CharacterVector fnameMt, std::vector<long> indxNA,
                                std::vector<long> dims);
Eigen::MatrixXd calculateMMt_rcpp(Rcpp::CharacterVector f_name_ascii, double max_memory_in_Gbytes, int num_cores,
                                  Rcpp::NumericVector selected_loci, std::vector<long> dims, bool quiet, Rcpp::Function message);
Rcpp::List calculate_a_and_vara_rcpp(Rcpp::CharacterVector f_name_ascii, Rcpp::NumericVector selected_loci,
                                     Eigen::Map<Eigen::MatrixXd> inv_MMt_sqrt, Eigen::Map<Eigen::MatrixXd> dim_reduced_vara,
                                     double max_memory_in_Gbytes, std::vector<long> dims, Eigen::VectorXd a, bool quiet,
                                     Rcpp::Function message);
Eigen::MatrixXd calculate_reduced_a_rcpp(Rcpp::CharacterVector f_name_ascii, double varG, Eigen::Map<Eigen::MatrixXd> P,
                                         Eigen::Map<Eigen::MatrixXd> y, double max_memory_in_Gbytes, std::vector<long> dims,
                                         Rcpp::NumericVector selected_loci, bool quiet, Rcpp::Function message);
bool createM_ASCII_rcpp(Rcpp::CharacterVector f_name, Rcpp::CharacterVector f_name_ascii, Rcpp::CharacterVector type,
                        std::string AA, std::string AB, std::string BB, double max_memory_in_Gbytes, std::vector<long> dims,
                        bool quiet, Rcpp::Function message, std::string missing);
void createMt_ASCII_rcpp(Rcpp::CharacterVector f_name, Rcpp::CharacterVector f_name_ascii, Rcpp::CharacterVector type,
                         double max_memory_in_Gbytes, std::vector<long> dims, bool quiet, Rcpp::Function message);
Eigen::VectorXi extract_geno_rcpp(Rcpp::CharacterVector f_name_ascii, double max_memory_in_Gbytes, long selected_locus,
                                  std::vector<long> dims);
std::vector<long> getRowColumn(std::string fname);
bool CreateASCIInospace(std::string fname, std::string asciifname, std::vector<long> dims, std::string AA, std::string AB,
                        std::string BB, bool quiet, Rcpp::Function message, std::string missing);
bool CreateASCIInospace_PLINK(std::string fname, std::string asciifname, std::vector<long> dims, bool quiet,
                              Rcpp::Function message);

namespace {
thread_local std::string g_error;

template <class F> int guarded(F f) {
    g_error.clear();
    try {
        f();
        return 0;
    } catch (const Rcpp::exception& e) {
        g_error = e.what();
        return -1;
    } catch (const std::exception& e) {
        g_error = e.what();
        return -2;
    }
}
std::vector<long> dims2(long a, long b) {
    std::vector<long> d(2);
    d[0] = a;
    d[1] = b;
    return d;
}
Eigen::Map<Eigen::MatrixXd> map(const double* p, long r, long c) { return Eigen::Map<Eigen::MatrixXd>(const_cast<double*>(p), r, c); }
template <class M> void copy_out(const M& m, double* out) {
    for (long j = 0; j < m.cols(); j++)
        for (long i = 0; i < m.rows(); i++) out[i + j * m.rows()] = m(i, j);
}
}  // namespace

extern "C" {

const char* er_last_error() { return g_error.c_str(); }
long er_message_count() { return (long)Rcpp::refstub_messages().size(); }
const char* er_message(long i) { return Rcpp::refstub_messages().at((size_t)i).c_str(); }
void er_clear_messages() { Rcpp::refstub_messages().clear(); }
int er_acc_is_long_double() { return sizeof(eagle_ref_acc) > sizeof(double); }

int er_ReadBlock(const char* path, long start_row, long numcols, long numrows, double* out_colmajor) {
    return guarded([&] { copy_out(ReadBlock(path, start_row, numcols, numrows), out_colmajor); });
}

int er_calculateMMt(const char* path, double max_memory_in_Gbytes, int num_cores, const double* sel, long nsel, long n, long L,
                    int quiet, double* out_colmajor) {
    return guarded([&] {
        copy_out(calculateMMt_rcpp(path, max_memory_in_Gbytes, num_cores, Rcpp::NumericVector(sel, nsel), dims2(n, L), quiet != 0,
                                   Rcpp::Function()),
                 out_colmajor);
    });
}

// a_out and vara_out hold L doubles; *out_len is the length the reference returned (1 for its sentinel List(a=0, vara=0)).
int er_calculate_a_and_vara(const char* path, const double* sel, long nsel, const double* S, const double* V,
                            double max_memory_in_Gbytes, long L, long n, const double* ahat, int quiet, double* a_out,
                            double* vara_out, long* out_len) {
    return guarded([&] {
        Eigen::VectorXd a(n);
        for (long i = 0; i < n; i++) a(i) = ahat[i];
        Rcpp::List res = calculate_a_and_vara_rcpp(path, Rcpp::NumericVector(sel, nsel), map(S, n, n), map(V, n, n),
                                                   max_memory_in_Gbytes, dims2(L, n), a, quiet != 0, Rcpp::Function());
        const std::vector<Rcpp::List::Item>& it = res.items();
        if (it.size() != 2 || it[0].name != "a" || it[1].name != "vara" || it[0].values.size() != it[1].values.size() ||
            (long)it[0].values.size() > L)
            throw std::logic_error("refstub: unexpected List from calculate_a_and_vara_rcpp");
        *out_len = (long)it[0].values.size();
        for (long i = 0; i < *out_len; i++) {
            a_out[i] = it[0].values[(size_t)i];
            vara_out[i] = it[1].values[(size_t)i];
        }
    });
}

// out holds max(L, 1) doubles; *out_len is rows() of what the reference returned (1 for its 1 x 1 null matrix).
int er_calculate_reduced_a(const char* path, double varG, const double* P, const double* y, double max_memory_in_Gbytes, long n,
                           long L, const double* sel, long nsel, int quiet, double* out, long* out_len) {
    return guarded([&] {
        Eigen::MatrixXd ar = calculate_reduced_a_rcpp(path, varG, map(P, n, n), map(y, n, 1), max_memory_in_Gbytes, dims2(n, L),
                                                      Rcpp::NumericVector(sel, nsel), quiet != 0, Rcpp::Function());
        if (ar.cols() != 1 || ar.rows() > (L > 1 ? L : 1)) throw std::logic_error("refstub: unexpected shape from calculate_reduced_a_rcpp");
        *out_len = ar.rows();
        copy_out(ar, out);
    });
}

int er_extract_geno(const char* path, double max_memory_in_Gbytes, long selected_locus, long n, long L, int* out) {
    return guarded([&] {
        Eigen::VectorXi g = extract_geno_rcpp(path, max_memory_in_Gbytes, selected_locus, dims2(n, L));
        if (g.size() != n) throw std::logic_error("refstub: unexpected length from extract_geno_rcpp");
        for (long i = 0; i < n; i++) out[i] = g(i);
    });
}

int er_getRowColumn(const char* path, long* dims_out) {
    return guarded([&] {
        std::vector<long> d = getRowColumn(path);
        dims_out[0] = d.at(0);
        dims_out[1] = d.at(1);
    });
}

int er_createM_ASCII(const char* f_name, const char* f_name_ascii, const char* type, const char* AA, const char* AB,
                     const char* BB, double max_memory_in_Gbytes, long d0, long d1, int quiet, const char* missing, int* it_worked) {
    return guarded([&] {
        *it_worked = createM_ASCII_rcpp(f_name, f_name_ascii, type, AA, AB, BB, max_memory_in_Gbytes, dims2(d0, d1), quiet != 0,
                                        Rcpp::Function(), missing)
                         ? 1
                         : 0;
    });
}

int er_CreateASCIInospace(const char* fname, const char* asciifname, long d0, long d1, const char* AA, const char* AB,
                          const char* BB, int quiet, const char* missing, int* it_worked) {
    return guarded([&] {
        *it_worked = CreateASCIInospace(fname, asciifname, dims2(d0, d1), AA, AB, BB, quiet != 0, Rcpp::Function(), missing) ? 1 : 0;
    });
}

int er_CreateASCIInospace_PLINK(const char* fname, const char* asciifname, long d0, long d1, int quiet, int* it_worked) {
    return guarded(
        [&] { *it_worked = CreateASCIInospace_PLINK(fname, asciifname, dims2(d0, d1), quiet != 0, Rcpp::Function()) ? 1 : 0; });
}

int er_createMt_ASCII(const char* f_name, const char* f_name_ascii, const char* type, double max_memory_in_Gbytes, long d0, long d1,
                      int quiet) {
    return guarded([&] {
        createMt_ASCII_rcpp(f_name, f_name_ascii, type, max_memory_in_Gbytes, dims2(d0, d1), quiet != 0, Rcpp::Function());
    });
}

int er_ReshapeM(const char* fnameM, const char* fnameMt, const long* indxNA, long n_na, long d0, long d1, long* newdims) {
    return guarded([&] {
        std::vector<long> nd = ReshapeM_rcpp(fnameM, fnameMt, std::vector<long>(indxNA, indxNA + n_na), dims2(d0, d1));
        newdims[0] = nd.at(0);
        newdims[1] = nd.at(1);
    });
}

}  // extern "C"

// TEST INFRASTRUCTURE ONLY.  A *functional* stand-in for the part of Eigen and Rcpp that the reference's
// src/*.cpp touch, so that those translation units compile unmodified and run without R (oracle/Makefile, target `ref`).
// Everything here is this project's own code: plain loops, eager evaluation.
//
// What is stood in for, and how:
//   * Eigen::Matrix<T>: column-major dense storage; (i,j), (i), rows(), cols(), resize, conservativeResize, setZero, Zero,
//     row(i) / col(j) / block(...) as assignable views, transpose(), noalias(), cast<U>(), scalar * matrix, matrix * matrix.
//   * A product is ALWAYS evaluated into a fresh temporary before it is assigned, so `x = A * x` behaves as in Eigen
//     (which also evaluates a product into a temporary unless noalias() is used, and the reference never uses noalias() on an
//     aliased operand).
//   * Products accumulate in the order i, j, k (k innermost, ascending) in the type eagle_ref_acc: double by default,
//     long double with -DEAGLE_REF_ACC_LONG_DOUBLE.  Each element is rounded to the matrix scalar once, at the end of its sum.
//     With long double, scalar * matrix is formed in long double as well.
//   * A 1 x 1 result converts to its scalar (Eigen's inner product rule), which is how `row * row.transpose()` is used.
//   * Eigen::initParallel / setNbThreads: no-ops; the stand-in is single threaded so results do not depend on a thread count.
//   * Rcpp: see Rcpp.h next to this file.
// What is NOT pinned by a build on this header: Eigen's own summation order and vectorisation, and anything R does.
#ifndef EAGLE_REFSTUB_RCPPEIGEN_H
#define EAGLE_REFSTUB_RCPPEIGEN_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <istream>
#include <iterator>
#include <limits>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "Rcpp.h"

#ifdef EAGLE_REF_ACC_LONG_DOUBLE
typedef long double eagle_ref_acc;
#else
typedef double eagle_ref_acc;
#endif

namespace Eigen {

[[noreturn]] inline void refstub_fail(const char* what) { throw std::out_of_range(std::string("refstub: ") + what); }
// Bounds are checked always: an out-of-range access in the reference is undefined there and must not pass silently here.
inline void refstub_check(bool ok, const char* what) {
    if (!ok) refstub_fail(what);
}

template <class T> class Matrix;

// A strided window onto storage owned by someone else: what row(), col(), block(), transpose() and Map hand out.
template <class T> class View {
  public:
    View(T* p, long r, long c, long rs, long cs) : p_(p), r_(r), c_(c), rs_(rs), cs_(cs) {}
    long rows() const { return r_; }
    long cols() const { return c_; }
    long size() const { return r_ * c_; }
    T& operator()(long i, long j) const {
        refstub_check(i >= 0 && i < r_ && j >= 0 && j < c_, "index (i,j) out of range");
        return p_[i * rs_ + j * cs_];
    }
    T& operator()(long i) const {
        refstub_check((r_ == 1 || c_ == 1) && i >= 0 && i < r_ * c_, "index (i) out of range");
        return r_ == 1 ? p_[i * cs_] : p_[i * rs_];
    }
    View transpose() const { return View(p_, c_, r_, cs_, rs_); }
    View row(long i) const {
        refstub_check(i >= 0 && i < r_, "row() out of range");
        return View(p_ + i * rs_, 1, c_, rs_, cs_);
    }
    View col(long j) const {
        refstub_check(j >= 0 && j < c_, "col() out of range");
        return View(p_ + j * cs_, r_, 1, rs_, cs_);
    }
    View block(long i, long j, long nr, long nc) const {
        refstub_check(i >= 0 && j >= 0 && nr >= 0 && nc >= 0 && i + nr <= r_ && j + nc <= c_, "block() out of range");
        return View(p_ + i * rs_ + j * cs_, nr, nc, rs_, cs_);
    }
    const View& setZero() const {
        for (long j = 0; j < c_; j++)
            for (long i = 0; i < r_; i++) p_[i * rs_ + j * cs_] = T(0);
        return *this;
    }
    View& noalias() { return *this; }
    // assignment writes through; the source is copied first because two views may overlap (removeRow, removeColumn)
    const View& operator=(const Matrix<T>& m) const;
    const View& operator=(const View& v) const;
    template <class U> Matrix<U> cast() const;
    operator T() const {
        refstub_check(r_ == 1 && c_ == 1, "only a 1 x 1 result converts to a scalar");
        return p_[0];
    }

  private:
    T* p_;
    long r_, c_, rs_, cs_;
};

template <class T> class Matrix {
  public:
    typedef T Scalar;
    Matrix() : r_(0), c_(0) {}
    Matrix(long r, long c) : r_(r), c_(c), d_(alloc(r, c)) {}
    explicit Matrix(long n) : r_(n), c_(1), d_(alloc(n, 1)) {}
    Matrix(const View<T>& v) : r_(v.rows()), c_(v.cols()), d_(alloc(v.rows(), v.cols())) {
        for (long j = 0; j < c_; j++)
            for (long i = 0; i < r_; i++) d_[i + j * r_] = v(i, j);
    }
    static Matrix Zero(long r, long c) {
        Matrix m(r, c);
        m.setZero();
        return m;
    }
    long rows() const { return r_; }
    long cols() const { return c_; }
    long size() const { return r_ * c_; }
    T* data() { return d_.data(); }
    const T* data() const { return d_.data(); }
    T& operator()(long i, long j) { return view()(i, j); }
    const T& operator()(long i, long j) const { return view()(i, j); }
    T& operator()(long i) { return view()(i); }
    const T& operator()(long i) const { return view()(i); }
    void resize(long r, long c) {  // values are not kept, as in Eigen
        r_ = r;
        c_ = c;
        d_ = alloc(r, c);
    }
    void conservativeResize(long r, long c) {
        Matrix m(r, c);
        m.setZero();
        for (long j = 0; j < std::min(c, c_); j++)
            for (long i = 0; i < std::min(r, r_); i++) m.d_[i + j * r] = d_[i + j * r_];
        *this = m;
    }
    Matrix& setZero() {
        std::fill(d_.begin(), d_.end(), T(0));
        return *this;
    }
    Matrix& noalias() { return *this; }
    View<T> view() const { return View<T>(const_cast<T*>(d_.data()), r_, c_, 1, r_); }
    View<T> row(long i) const { return view().row(i); }
    View<T> col(long j) const { return view().col(j); }
    View<T> block(long i, long j, long nr, long nc) const { return view().block(i, j, nr, nc); }
    View<T> transpose() const { return view().transpose(); }
    template <class U> Matrix<U> cast() const { return view().template cast<U>(); }
    Matrix& operator=(const View<T>& v) {
        Matrix m(v);
        r_ = m.r_;
        c_ = m.c_;
        d_.swap(m.d_);
        return *this;
    }
    operator T() const { return T(view()); }

  private:
    static std::vector<T> alloc(long r, long c) {
        refstub_check(r >= 0 && c >= 0, "negative matrix dimension");
        return std::vector<T>((size_t)r * (size_t)c);
    }
    long r_, c_;
    std::vector<T> d_;
};

template <class T> const View<T>& View<T>::operator=(const Matrix<T>& m) const {
    refstub_check(m.rows() == r_ && m.cols() == c_, "assignment to a view of another shape");
    for (long j = 0; j < c_; j++)
        for (long i = 0; i < r_; i++) p_[i * rs_ + j * cs_] = m(i, j);
    return *this;
}
template <class T> const View<T>& View<T>::operator=(const View<T>& v) const { return *this = Matrix<T>(v); }
template <class T> template <class U> Matrix<U> View<T>::cast() const {
    Matrix<U> m(r_, c_);
    for (long j = 0; j < c_; j++)
        for (long i = 0; i < r_; i++) m(i, j) = static_cast<U>((*this)(i, j));
    return m;
}

// Map<MatrixXd>: the caller's column-major memory, not copied.
template <class M> class Map : public View<typename M::Scalar> {
  public:
    typedef typename M::Scalar Scalar;
    Map(Scalar* p, long r, long c) : View<Scalar>(p, r, c, 1, r) {}
    Map(Scalar* p, long n) : View<Scalar>(p, n, 1, 1, n) {}
};

// C = A * B, order i, j, k, one rounding per element.
template <class T> Matrix<T> refstub_product(const View<T>& a, const View<T>& b) {
    refstub_check(a.cols() == b.rows(), "product of mismatched shapes");
    const long m = a.rows(), n = b.cols(), kk = a.cols();
    Matrix<T> c(m, n);
    for (long i = 0; i < m; i++)
        for (long j = 0; j < n; j++) {
            eagle_ref_acc s = 0;
            for (long k = 0; k < kk; k++) s += (eagle_ref_acc)a(i, k) * (eagle_ref_acc)b(k, j);
            c(i, j) = (T)s;
        }
    return c;
}
template <class T> Matrix<T> operator*(const Matrix<T>& a, const Matrix<T>& b) { return refstub_product(a.view(), b.view()); }
template <class T> Matrix<T> operator*(const Matrix<T>& a, const View<T>& b) { return refstub_product(a.view(), b); }
template <class T> Matrix<T> operator*(const View<T>& a, const Matrix<T>& b) { return refstub_product(a, b.view()); }
template <class T> Matrix<T> operator*(const View<T>& a, const View<T>& b) { return refstub_product(a, b); }
// (a Map is a View by inheritance and takes the View overloads)
template <class T> Matrix<T> operator*(double s, const Matrix<T>& a) {
    Matrix<T> c(a.rows(), a.cols());
    for (long j = 0; j < a.cols(); j++)
        for (long i = 0; i < a.rows(); i++) c(i, j) = (T)((eagle_ref_acc)s * (eagle_ref_acc)a(i, j));
    return c;
}

typedef Matrix<double> MatrixXd;
typedef Matrix<int> MatrixXi;
typedef Matrix<double> VectorXd;
typedef Matrix<int> VectorXi;

inline void initParallel() {}
inline void setNbThreads(int) {}

}  // namespace Eigen
#endif

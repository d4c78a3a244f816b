// TEST INFRASTRUCTURE ONLY.  Functional stand-in for the few Rcpp names the reference's src/*.cpp use (see RcppEigen.h
// next to this file).  This project's own code.
//
//   * Rcpp::stop(text) throws Rcpp::exception carrying the text.
//   * Rcpp::Function stands for R's message(): it pastes its arguments with no separator and appends the line to a
//     buffer (refstub_messages()).  Strings are taken as they are, integers in decimal, doubles with up to 15 significant
//     digits (R's as.character default), a CharacterVector as its first element.
//   * R_IsNA(x): true for R's NA_real_ -- a NaN whose low 32 bits are 1954 -- and ALSO for any other NaN.  R itself tells
//     the two apart; a non-NA NaN in selected_loci is an index the reference cannot use, and every caller of this
//     project passes numpy's NaN for NA.
//   * Rcpp::Rcout swallows what is written to it (the reference prints a progress line to it).
//   * List::create(Named(..) = ..) keeps (name, matrix) pairs; a scalar value becomes a 1 x 1 matrix.
#ifndef EAGLE_REFSTUB_RCPP_H
#define EAGLE_REFSTUB_RCPP_H

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

inline bool R_IsNA(double x) {
    // R's rule is isnan(x) && low word == 1954; the wider rule of the header comment makes the payload test redundant
    return std::isnan(x);
}

namespace Eigen {
template <class T> class Matrix;
}

namespace Rcpp {

class exception : public std::runtime_error {
  public:
    explicit exception(const std::string& s) : std::runtime_error(s) {}
};
[[noreturn]] inline void stop(const std::string& text) { throw exception(text); }

class CharacterVector {
  public:
    CharacterVector() {}
    CharacterVector(const char* s) : v_(1, std::string(s)) {}
    CharacterVector(const std::string& s) : v_(1, s) {}
    const std::string& first() const {
        static const std::string empty;
        return v_.empty() ? empty : v_[0];
    }

  private:
    std::vector<std::string> v_;
};
template <class T> T as(const CharacterVector& c) { return T(c.first()); }

class NumericVector {
  public:
    NumericVector() {}
    NumericVector(const double* p, long n) : v_(p, p + n) {}
    double operator()(long i) const {
        if (i < 0 || i >= (long)v_.size()) throw std::out_of_range("refstub: NumericVector index out of range");
        return v_[i];
    }
    double operator[](long i) const { return (*this)(i); }
    long size() const { return (long)v_.size(); }

  private:
    std::vector<double> v_;
};

inline std::vector<std::string>& refstub_messages() {
    static thread_local std::vector<std::string> buf;
    return buf;
}

class Function {
  public:
    Function() {}
    template <class... A> void operator()(const A&... args) const {
        std::string line;
        paste(line, args...);
        refstub_messages().push_back(line);
    }

  private:
    static void paste(std::string&) {}
    template <class H, class... R> static void paste(std::string& s, const H& h, const R&... rest) {
        one(s, h);
        paste(s, rest...);
    }
    static void one(std::string& s, const char* t) { s += t; }
    static void one(std::string& s, const std::string& t) { s += t; }
    static void one(std::string& s, const CharacterVector& t) { s += t.first(); }
    static void one(std::string& s, int v) { s += std::to_string(v); }
    static void one(std::string& s, long v) { s += std::to_string(v); }
    static void one(std::string& s, unsigned long v) { s += std::to_string(v); }
    static void one(std::string& s, double v) {
        char b[64];
        std::snprintf(b, sizeof b, "%.15g", v);
        s += b;
    }
};

class NullStream : public std::ostream {
    class Buf : public std::streambuf {
        int overflow(int c) override { return c; }
    } buf_;

  public:
    NullStream() : std::ostream(&buf_) {}
};
static NullStream Rcout;

template <class T> struct NamedValue {
    std::string name;
    const T& value;
};
class Named {
  public:
    explicit Named(const char* n) : n_(n) {}
    template <class T> NamedValue<T> operator=(const T& v) const { return NamedValue<T>{n_, v}; }

  private:
    std::string n_;
};

class List {
  public:
    struct Item {
        std::string name;
        long rows, cols;
        std::vector<double> values;  // column-major
    };
    template <class... A> static List create(const A&... a) {
        List l;
        l.add(a...);
        return l;
    }
    const std::vector<Item>& items() const { return items_; }

  private:
    void add() {}
    template <class H, class... R> void add(const H& h, const R&... rest) {
        items_.push_back(item(h.name, h.value));
        add(rest...);
    }
    static Item item(const std::string& n, int v) { return Item{n, 1, 1, std::vector<double>(1, (double)v)}; }
    static Item item(const std::string& n, double v) { return Item{n, 1, 1, std::vector<double>(1, v)}; }
    template <class M> static Item item(const std::string& n, const M& m) {
        Item it{n, m.rows(), m.cols(), std::vector<double>()};
        it.values.reserve((size_t)(m.rows() * m.cols()));
        for (long j = 0; j < m.cols(); j++)
            for (long i = 0; i < m.rows(); i++) it.values.push_back(m(i, j));
        return it;
    }
    std::vector<Item> items_;
};

}  // namespace Rcpp
#endif

// flatten_node_columns.cc — object level -> the raw int64 node columns of NodeMetadata and PodState, and QOSSort's host side.
// Host-side product code (once per snapshot).
//
// What is hoisted out of the per-(pod, node) path, and where the reference does it per call:
//   NodeMetadata : calculateScore (node_metadata.go:80-104) reads one label or annotation of the node and parses it on EVERY Score call:
//                  strconv.ParseFloat (:108-122) or time.Parse + time.Since (:125-145)          -> one int64 per node, math.MinInt64 = invalid
//   PodState     : score (pod_state.go:52-64) walks the node's pods and the nominated pods on every call -> terminating - nominated per node
//   QOSSort      : Less (queue_sort.go:46-58) calls v1qos.GetPodQOS twice per comparison           -> the class once per pod
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#include "../../include/spx.h"
#include "nrt_release.hpp"

namespace {

constexpr int64_t kInvalid = std::numeric_limits<int64_t>::min();  // node_metadata.go:48

inline char lower(char c) { return (c >= 'A' && c <= 'Z') ? static_cast<char>(c - 'A' + 'a') : c; }
inline bool is_digit(char c) { return c >= '0' && c <= '9'; }
inline bool is_hex(char c) { return is_digit(c) || (lower(c) >= 'a' && lower(c) <= 'f'); }

size_t common_prefix_ci(const char* s, size_t n, const char* word) {
  size_t i = 0;
  while (i < n && word[i] && lower(s[i]) == word[i]) ++i;
  return i;
}

// strconv's special(): [+-]inf, [+-]infinity, nan (no sign), any case; the whole string
bool parse_special(const char* s, size_t n, double* out) {
  if (n == 0) return false;
  double sign = 1.0;
  size_t i = 0;
  if (s[0] == '+' || s[0] == '-') {
    sign = s[0] == '-' ? -1.0 : 1.0;
    i = 1;
    const size_t k = common_prefix_ci(s + i, n - i, "infinity");
    if ((k == 3 || k == 8) && i + k == n) return *out = sign * std::numeric_limits<double>::infinity(), true;
    return false;
  }
  if (lower(s[0]) == 'i') {
    const size_t k = common_prefix_ci(s, n, "infinity");
    if ((k == 3 || k == 8) && k == n) return *out = std::numeric_limits<double>::infinity(), true;
    return false;
  }
  if (lower(s[0]) == 'n' && n == 3 && common_prefix_ci(s, n, "nan") == 3) return *out = std::numeric_limits<double>::quiet_NaN(), true;
  return false;
}

// strconv.ParseFloat(s, 64): the grammar is checked here (readFloat's: sign, digits with at most one point and at least one digit,
// an exponent with at least one digit; 0x form with a mandatory p exponent and underscores between its digits), the value comes from
// strtod on the accepted text without its underscores — correctly rounded for both forms.  false = Go returns an error.
bool parse_float(const char* s, size_t n, double* out) {
  if (parse_special(s, n, out)) return true;
  std::string clean;
  clean.reserve(n + 1);
  size_t i = 0;
  if (i < n && (s[i] == '+' || s[i] == '-')) clean.push_back(s[i++]);
  const bool hex = i + 2 < n && s[i] == '0' && lower(s[i + 1]) == 'x';
  if (hex) {
    clean += "0x";
    i += 2;
  }
  // '0': a digit or the base prefix, '_': an underscore, '!': anything else, '^': the start (underscoreOK's states)
  char saw = hex ? '0' : '^';
  bool sawdot = false, sawdigits = false;
  for (; i < n; ++i) {
    const char c = s[i];
    if (c == '_') {
      if (!hex || saw != '0') return false;  // underscores only behind a base prefix, and only after a digit
      saw = '_';
      continue;
    }
    if (c == '.') {
      if (sawdot || saw == '_') return false;
      sawdot = true;
      saw = '!';
      clean.push_back(c);
      continue;
    }
    if (hex ? is_hex(c) : is_digit(c)) {
      sawdigits = true;
      saw = '0';
      clean.push_back(c);
      continue;
    }
    break;
  }
  if (!sawdigits || saw == '_') return false;
  bool sawexp = false;
  if (i < n && lower(s[i]) == (hex ? 'p' : 'e')) {
    clean.push_back(s[i++]);
    if (i < n && (s[i] == '+' || s[i] == '-')) clean.push_back(s[i++]);
    saw = '!';
    bool expdigits = false;
    for (; i < n; ++i) {
      const char c = s[i];
      if (c == '_') {
        if (!hex || saw != '0') return false;
        saw = '_';
        continue;
      }
      if (!is_digit(c)) break;
      expdigits = true;
      saw = '0';
      clean.push_back(c);
    }
    if (!expdigits || saw == '_') return false;
    sawexp = true;
  }
  if (i != n) return false;             // junk, blanks
  if (hex && !sawexp) return false;     // "hexadecimal mantissa requires a 'p' exponent"
  errno = 0;
  char* end = nullptr;
  const double v = std::strtod(clean.c_str(), &end);
  if (end != clean.c_str() + clean.size()) return false;
  if (std::isinf(v)) return false;      // ErrRange (an underflow to 0 is no error in Go)
  *out = v;
  return true;
}

// int64(v) as amd64's CVTTSD2SI gives it: NaN, +-Inf and |v| >= 2^63 -> math.MinInt64
inline int64_t go_int64(double v) {
  if (!(v >= -0x1p63 && v < 0x1p63)) return kInvalid;
  return static_cast<int64_t>(v);  // (-2^63 itself converts exactly: the same bits)
}
inline int64_t wrap_neg(int64_t v) { return static_cast<int64_t>(0 - static_cast<uint64_t>(v)); }

// ---- time.Parse(time.RFC3339, s) ----
bool two_digits(const char* s, size_t n, size_t& i, int* out) {
  if (i + 2 > n || !is_digit(s[i]) || !is_digit(s[i + 1])) return false;
  *out = (s[i] - '0') * 10 + (s[i + 1] - '0');
  i += 2;
  return true;
}
inline bool leap(int y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }
inline int days_in(int m, int y) {
  static const int d[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  return m == 2 && leap(y) ? 29 : d[m - 1];
}
// days from 1970-01-01 of a proleptic Gregorian date
inline int64_t days_from_civil(int64_t y, int m, int d) {
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const int64_t yoe = y - era * 400;
  const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

// seconds since the Unix epoch and nanoseconds of the instant; false = time.Parse returns an error
bool parse_rfc3339(const char* s, size_t n, int64_t* sec_out, int32_t* nsec_out) {
  size_t i = 0;
  if (n < 4 || !is_digit(s[0]) || !is_digit(s[1]) || !is_digit(s[2]) || !is_digit(s[3])) return false;
  const int year = (s[0] - '0') * 1000 + (s[1] - '0') * 100 + (s[2] - '0') * 10 + (s[3] - '0');
  i = 4;
  int month, day, hour, minute, second;
  if (i >= n || s[i++] != '-' || !two_digits(s, n, i, &month)) return false;
  if (i >= n || s[i++] != '-' || !two_digits(s, n, i, &day)) return false;
  if (i >= n || s[i++] != 'T') return false;
  // the layout's "15" takes one or two digits (getnum, not fixed)
  if (i >= n || !is_digit(s[i])) return false;
  hour = s[i++] - '0';
  if (i < n && is_digit(s[i])) hour = hour * 10 + (s[i++] - '0');
  if (i >= n || s[i++] != ':' || !two_digits(s, n, i, &minute)) return false;
  if (i >= n || s[i++] != ':' || !two_digits(s, n, i, &second)) return false;
  int64_t nsec = 0;
  if (i + 1 < n && (s[i] == '.' || s[i] == ',') && is_digit(s[i + 1])) {  // a fraction the layout does not name: any length, cut at 9 digits
    ++i;
    int digits = 0;
    for (; i < n && is_digit(s[i]); ++i)
      if (digits < 9) nsec = nsec * 10 + (s[i] - '0'), ++digits;
    for (; digits < 9; ++digits) nsec *= 10;
  }
  int64_t offset = 0;
  if (i < n && s[i] == 'Z') {
    ++i;
  } else {
    if (i >= n || (s[i] != '+' && s[i] != '-')) return false;
    const int sign = s[i++] == '-' ? -1 : 1;
    int oh, om;
    if (!two_digits(s, n, i, &oh) || i >= n || s[i++] != ':' || !two_digits(s, n, i, &om)) return false;
    if (oh > 24 || om > 60) return false;  // (Parse tests with >: "some people do write offsets of 24 hours or 60 minutes")
    offset = sign * (oh * 3600 + om * 60);
  }
  if (i != n) return false;  // "extra text"
  if (month < 1 || month > 12 || day < 1 || day > days_in(month, year) || hour >= 24 || minute >= 60 || second >= 60) return false;
  *sec_out = days_from_civil(year, month, day) * 86400 + hour * 3600 + minute * 60 + second - offset;
  *nsec_out = static_cast<int32_t>(nsec);
  return true;
}

// time.Since(t).Seconds() with an explicit now, then the strategy's int64 conversion (node_metadata.go:134-144).  Time.Sub saturates
// at the ends of time.Duration; Duration.Seconds() is float64(d / 1e9) + float64(d % 1e9) / 1e9.
int64_t age_score(int64_t now_ns, int64_t t_sec, int32_t t_nsec, int strategy) {
  const __int128 d128 = static_cast<__int128>(now_ns) - (static_cast<__int128>(t_sec) * 1000000000 + t_nsec);
  int64_t d;
  if (d128 > std::numeric_limits<int64_t>::max()) d = std::numeric_limits<int64_t>::max();
  else if (d128 < std::numeric_limits<int64_t>::min()) d = std::numeric_limits<int64_t>::min();
  else d = static_cast<int64_t>(d128);
  const double age = static_cast<double>(d / 1000000000) + static_cast<double>(d % 1000000000) / 1e9;
  const int64_t whole = go_int64(age);
  return strategy == SPX_NODEMETA_NEWEST ? wrap_neg(whole) : whole;
}

}  // namespace

extern "C" {

int spx_flatten_nodemeta(const char* values, const int64_t* value_ptr, const uint8_t* found, int64_t n_nodes, int type, int strategy, int64_t now_unix_nanos,
                         int64_t* raw_out) {
  if (n_nodes < 0 || !value_ptr || !found || !raw_out) return SPX_ERR_ARG;
  const bool number = type == SPX_NODEMETA_NUMBER;
  if (!number && type != SPX_NODEMETA_TIMESTAMP) return SPX_ERR_ARG;
  if (number ? (strategy != SPX_NODEMETA_HIGHEST && strategy != SPX_NODEMETA_LOWEST) : (strategy != SPX_NODEMETA_NEWEST && strategy != SPX_NODEMETA_OLDEST))
    return SPX_ERR_ARG;
  for (int64_t i = 0; i < n_nodes; ++i)
    if (value_ptr[i] < 0 || value_ptr[i + 1] < value_ptr[i]) return SPX_ERR_ARG;
  if (n_nodes > 0 && value_ptr[n_nodes] > 0 && !values) return SPX_ERR_ARG;
  for (int64_t i = 0; i < n_nodes; ++i) {
    raw_out[i] = kInvalid;
    if (!found[i]) continue;
    const char* s = values + value_ptr[i];
    const size_t n = static_cast<size_t>(value_ptr[i + 1] - value_ptr[i]);
    if (number) {
      double v;
      if (!parse_float(s, n, &v)) continue;
      const int64_t score = go_int64(v);
      raw_out[i] = strategy == SPX_NODEMETA_LOWEST ? wrap_neg(score) : score;
    } else {
      int64_t sec;
      int32_t nsec;
      if (!parse_rfc3339(s, n, &sec, &nsec)) continue;
      raw_out[i] = age_score(now_unix_nanos, sec, nsec, strategy);
    }
  }
  return SPX_OK;
}

int spx_flatten_nodemeta_unix(const int64_t* unix_nanos, const uint8_t* valid, int64_t n_nodes, int strategy, int64_t now_unix_nanos, int64_t* raw_out) {
  if (n_nodes < 0 || !unix_nanos || !valid || !raw_out) return SPX_ERR_ARG;
  if (strategy != SPX_NODEMETA_NEWEST && strategy != SPX_NODEMETA_OLDEST) return SPX_ERR_ARG;
  for (int64_t i = 0; i < n_nodes; ++i) {
    if (!valid[i]) {
      raw_out[i] = kInvalid;
      continue;
    }
    int64_t sec = unix_nanos[i] / 1000000000;
    int64_t nsec = unix_nanos[i] % 1000000000;
    if (nsec < 0) nsec += 1000000000, --sec;
    raw_out[i] = age_score(now_unix_nanos, sec, static_cast<int32_t>(nsec), strategy);
  }
  return SPX_OK;
}

int spx_flatten_podstate(int64_t n_nodes, int64_t n_assigned, const int64_t* assigned_node, const uint8_t* assigned_terminating, int64_t n_nominated,
                         const int64_t* nominated_node, int64_t* raw_out) {
  if (n_nodes < 0 || n_assigned < 0 || n_nominated < 0 || !raw_out) return SPX_ERR_ARG;
  if ((n_assigned > 0 && (!assigned_node || !assigned_terminating)) || (n_nominated > 0 && !nominated_node)) return SPX_ERR_ARG;
  for (int64_t i = 0; i < n_assigned; ++i)
    if (assigned_node[i] < 0 || assigned_node[i] >= n_nodes) return SPX_ERR_ARG;
  for (int64_t i = 0; i < n_nominated; ++i)
    if (nominated_node[i] < 0 || nominated_node[i] >= n_nodes) return SPX_ERR_ARG;
  for (int64_t n = 0; n < n_nodes; ++n) raw_out[n] = 0;
  for (int64_t i = 0; i < n_assigned; ++i)
    if (assigned_terminating[i]) ++raw_out[assigned_node[i]];  // DeletionTimestamp != nil, pod_state.go:59-61
  for (int64_t i = 0; i < n_nominated; ++i) --raw_out[nominated_node[i]];  // len(NominatedPodsForNode), :56
  return SPX_OK;
}

int spx_flatten_pod_qos(const spx_pod_objects* pods, uint8_t* qos_out) {
  if (!pods || !qos_out) return SPX_ERR_ARG;
  for (int64_t i = 0; i < pods->n_pods; ++i) {
    const int q = spx_host::nrt_pod_qos(pods, i);
    qos_out[i] = q == SPX_QOS_GUARANTEED ? SPX_QOSSORT_GUARANTEED : (q == SPX_QOS_BURSTABLE ? SPX_QOSSORT_BURSTABLE : SPX_QOSSORT_BEST_EFFORT);
  }
  return SPX_OK;
}

int spx_qos_less(int32_t priority1, int qos1, int64_t ts1, int32_t priority2, int qos2, int64_t ts2) {
  if (priority1 != priority2) return priority1 > priority2;
  if (qos1 != qos2) return qos1 > qos2;
  return ts1 < ts2;
}

}  // extern "C"

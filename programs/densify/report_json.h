// report_json.h -- the text of the densify CLI's report: numbers in the
// report's formats and an ordered JSON object that grows a std::string.  It
// writes only (dpio::Json reads); no GPU, nothing of the library.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

// v as printf's %.<digits>g or, fixed, %.<digits>f, at whatever length that takes
inline std::string decimal(double v, int digits, bool fixed = false)
{
    auto print = [&](char *to, size_t n) {
        return fixed ? std::snprintf(to, n, "%.*f", digits, v) : std::snprintf(to, n, "%.*g", digits, v);
    };
    std::string s((size_t)print(nullptr, 0), '\0');
    print(&s[0], s.size() + 1);
    return s;
}

// %.17g, which reads back to the same double; null for a value that is not finite
inline std::string number(double v)
{
    return std::isfinite(v) ? decimal(v, 17) : "null";
}

// [a, b, ...] of values that are JSON text already
inline std::string json_array(const std::vector<std::string> &values)
{
    std::string s = "[";
    for (size_t i = 0; i < values.size(); ++i)
        (s += i ? ", " : "") += values[i];
    return s + "]";
}

// The members of one object in the order they were added, one method per
// format of the report.  Keys and strings are written as they are given.
class JsonObject {
    std::string text; // the members, without the braces

    JsonObject &member(const char *key, const std::string &value)
    {
        (((text += text.empty() ? "\"" : ", \"") += key) += "\": ") += value;
        return *this;
    }

public:
    template <typename T> JsonObject &integer(const char *key, T v)
    {
        static_assert(std::is_integral<T>::value && !std::is_same<T, bool>::value, "integer() takes an integer");
        return member(key, std::to_string(v));
    }
    JsonObject &ms(const char *key, double v) { return member(key, decimal(v, 3, true)); } // %.3f
    JsonObject &g9(const char *key, double v) { return member(key, decimal(v, 9)); }       // %.9g
    JsonObject &g17(const char *key, double v) { return member(key, number(v)); }          // %.17g or null
    JsonObject &boolean(const char *key, bool v) { return member(key, v ? "true" : "false"); }
    JsonObject &string(const char *key, const std::string &v) { return member(key, "\"" + v + "\""); }
    JsonObject &object(const char *key, const JsonObject &o) { return member(key, o.str()); }
    // a value that is JSON text already (json_array of objects or strings)
    JsonObject &raw(const char *key, const std::string &json) { return member(key, json); }
    // n numbers: integers as integer() writes them, doubles as g17() does
    template <typename T> JsonObject &array(const char *key, const T *v, size_t n)
    {
        std::vector<std::string> values;
        for (size_t i = 0; i < n; ++i)
            if constexpr (std::is_integral<T>::value)
                values.push_back(std::to_string(v[i]));
            else
                values.push_back(number(v[i]));
        return member(key, json_array(values));
    }
    // o's members after these, as siblings
    JsonObject &members(const JsonObject &o)
    {
        if (!o.text.empty())
            (text += text.empty() ? "" : ", ") += o.text;
        return *this;
    }
    bool empty() const { return text.empty(); }
    std::string str() const { return "{" + text + "}"; }
};

// cli_error.h -- how a stage of the densify CLI fails: it throws the message
// that main prints after "densify: " before it exits with 1, so every owner on
// the way out releases what it holds.
#pragma once

#include <stdexcept>
#include <string>

struct CliError : std::runtime_error {
    using std::runtime_error::runtime_error;
    // "<what> failed (<rc>): <detail>", or with `where` "<what> failed <where> (<rc>): <detail>"
    CliError(const std::string &what, int rc, const std::string &detail, const std::string &where = "")
        : std::runtime_error(what + " failed " + (where.empty() ? "" : where + " ") + "(" + std::to_string(rc) +
                             "): " + detail)
    {
    }
};

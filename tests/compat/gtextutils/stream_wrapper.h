// Test-only stand-in for <gtextutils/stream_wrapper.h>: the two classes fasta_formatter.cpp uses, written for this project.
// An empty file name means the standard stream; a file that cannot be opened ends the program with status 1.
#ifndef FXG_TEST_COMPAT_STREAM_WRAPPER_H
#define FXG_TEST_COMPAT_STREAM_WRAPPER_H
#include <err.h>
#include <fstream>
#include <iostream>
#include <string>

class InputStreamWrapper {
    std::ifstream file_;
    bool use_file_;

public:
    explicit InputStreamWrapper(const std::string &name) : use_file_(!name.empty())
    {
        if (use_file_) {
            file_.open(name.c_str(), std::ios::in | std::ios::binary);
            if (!file_) errx(1, "failed to open input file '%s'", name.c_str());
        }
    }
    std::istream &stream() { return use_file_ ? static_cast<std::istream &>(file_) : std::cin; }
};

class OutputStreamWrapper {
    std::ofstream file_;
    bool use_file_;

public:
    explicit OutputStreamWrapper(const std::string &name) : use_file_(!name.empty())
    {
        if (use_file_) {
            file_.open(name.c_str(), std::ios::out | std::ios::binary | std::ios::trunc);
            if (!file_) errx(1, "failed to create output file '%s'", name.c_str());
        }
    }
    std::ostream &stream() { return use_file_ ? static_cast<std::ostream &>(file_) : std::cout; }
};
#endif

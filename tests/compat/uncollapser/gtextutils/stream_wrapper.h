// Test-only stand-in for <gtextutils/stream_wrapper.h>, written for this project: just enough for the reference's fastx_uncollapser.cpp to compile.
// Only its tabular mode (-c), which no test runs, uses these classes.
#ifndef FXG_TEST_COMPAT_UC_STREAM_WRAPPER_H
#define FXG_TEST_COMPAT_UC_STREAM_WRAPPER_H
#include <fstream>
#include <iostream>
#include <string>

class InputStreamWrapper {
    std::ifstream file_;
    bool use_file_;

public:
    explicit InputStreamWrapper(const std::string &name) : use_file_(!name.empty()) { if (use_file_) file_.open(name.c_str()); }
    std::istream &stream() { return use_file_ ? static_cast<std::istream &>(file_) : std::cin; }
};

class OutputStreamWrapper {
    std::ofstream file_;
    bool use_file_;

public:
    explicit OutputStreamWrapper(const std::string &name) : use_file_(!name.empty()) { if (use_file_) file_.open(name.c_str()); }
    std::ostream &stream() { return use_file_ ? static_cast<std::ostream &>(file_) : std::cout; }
};
#endif

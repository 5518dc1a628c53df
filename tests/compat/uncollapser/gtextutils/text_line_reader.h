// Test-only stand-in for <gtextutils/text_line_reader.h>, written for this project: std::getline with a line count, which is what
// fastx_uncollapser.cpp's tabular mode asks of it.
#ifndef FXG_TEST_COMPAT_UC_TEXT_LINE_READER_H
#define FXG_TEST_COMPAT_UC_TEXT_LINE_READER_H
#include <cstddef>
#include <istream>
#include <string>

class TextLineReader {
    std::istream &in_;
    std::string line_;
    size_t number_;

public:
    explicit TextLineReader(std::istream &in) : in_(in), number_(0) {}
    bool next_line() { if (!std::getline(in_, line_)) return false; ++number_; return true; }
    const std::string &line_string() const { return line_; }
    size_t line_number() const { return number_; }
};
#endif

// Test-only stand-in for <gtextutils/text_line_reader.h>: a line reader that is std::getline, written for this project.
#ifndef FXG_TEST_COMPAT_TEXT_LINE_READER_H
#define FXG_TEST_COMPAT_TEXT_LINE_READER_H
#include <istream>
#include <string>

class TextLineReader {
    std::istream &in_;
    std::string line_;

public:
    explicit TextLineReader(std::istream &in) : in_(in) {}
    bool next_line() { return static_cast<bool>(std::getline(in_, line_)); }
    const std::string &line_string() const { return line_; }
};
#endif

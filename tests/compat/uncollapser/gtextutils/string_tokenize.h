// Test-only stand-in for <gtextutils/string_tokenize.h>, written for this project so that fastx_uncollapser.cpp compiles.  It cuts at every
// delimiter byte; what libgtextutils does with empty fields is not known here, which is why no test runs the tabular mode.
#ifndef FXG_TEST_COMPAT_UC_STRING_TOKENIZE_H
#define FXG_TEST_COMPAT_UC_STRING_TOKENIZE_H
#include <string>

template <typename OutputIterator>
void String_Tokenize(const std::string &text, OutputIterator out, const std::string &delimiters)
{
    std::string::size_type from = 0;
    for (;;) {
        const std::string::size_type at = text.find_first_of(delimiters, from);
        *out++ = text.substr(from, at == std::string::npos ? std::string::npos : at - from);
        if (at == std::string::npos) return;
        from = at + 1;
    }
}
#endif

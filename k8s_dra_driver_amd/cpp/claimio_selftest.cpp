// Stand-alone self-test of claimio_core.hpp, meant to be built with
// -fsanitize=address,undefined and run directly (no Python involved):
//
//   g++ -g -O1 -std=c++17 -fsanitize=address,undefined \
//       claimio_selftest.cpp -o claimio_selftest && ./claimio_selftest
//
// Exit status 0 and a final "claimio_selftest: OK" line mean every check
// passed and neither sanitizer reported anything.

#include "claimio_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <dirent.h>
#include <sys/stat.h>

static int g_failures = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__,     \
                         #cond);                                             \
            ++g_failures;                                                    \
        }                                                                    \
    } while (0)

// ---------------------------------------------------------------------------
// escaper: an independent, deliberately naive rendering of the same rules
// ---------------------------------------------------------------------------

static std::string ref_escape_cp(uint32_t c) {
    char buf[16];
    switch (c) {
        case '"': return "\\\"";
        case '\\': return "\\\\";
        case '\n': return "\\n";
        case '\r': return "\\r";
        case '\t': return "\\t";
        case '\b': return "\\b";
        case '\f': return "\\f";
        default: break;
    }
    if (c < 0x20) {
        std::snprintf(buf, sizeof(buf), "\\u%04x", c);
        return buf;
    }
    if (c <= 0x7e) return std::string(1, static_cast<char>(c));
    if (c < 0x10000) {
        std::snprintf(buf, sizeof(buf), "\\u%04x", c);
        return buf;
    }
    uint32_t v = c - 0x10000;
    std::snprintf(buf, sizeof(buf), "\\u%04x\\u%04x", 0xd800 + (v >> 10),
                  0xdc00 + (v & 0x3ff));
    return buf;
}

template <typename CharT>
static void check_range(uint32_t lo, uint32_t hi) {
    // every code point on its own ...
    for (uint32_t c = lo; c <= hi; ++c) {
        CharT s[1] = {static_cast<CharT>(c)};
        std::string got;
        claimio::append_escaped(got, s, 1);
        std::string want = "\"" + ref_escape_cp(c) + "\"";
        if (got != want) {
            std::fprintf(stderr, "FAIL escape U+%04X width %zu: %s != %s\n", c,
                         sizeof(CharT), got.c_str(), want.c_str());
            ++g_failures;
            return;
        }
    }
    // ... and all of them in one string, between plain runs
    std::vector<CharT> all;
    std::string want = "\"";
    for (uint32_t c = lo; c <= hi; ++c) {
        all.push_back(static_cast<CharT>('a'));
        all.push_back(static_cast<CharT>(c));
        want += "a" + ref_escape_cp(c);
    }
    want += "\"";
    std::string got;
    claimio::append_escaped(got, all.data(), all.size());
    CHECK(got == want);
}

static void test_escaper() {
    check_range<uint8_t>(0x00, 0xff);
    check_range<uint16_t>(0x0000, 0xffff);  // lone surrogates included
    check_range<uint32_t>(0x000000, 0x10ffff);

    std::string out;
    claimio::append_escaped(out, static_cast<const uint8_t*>(nullptr), 0);
    CHECK(out == "\"\"");

    // boundaries spelled out
    const uint32_t edges[] = {0x00,   0x1f,   0x20,   0x22,    0x5c,    0x7e,
                              0x7f,   0x80,   0xff,   0x100,   0x2028,  0xd7ff,
                              0xd800, 0xdbff, 0xdc00, 0xdfff,  0xe000,  0xffff,
                              0x10000, 0x1f600, 0x10ffff};
    out.clear();
    claimio::append_escaped(out, edges, sizeof(edges) / sizeof(edges[0]));
    CHECK(out ==
          "\"\\u0000\\u001f \\\"\\\\~\\u007f\\u0080\\u00ff\\u0100\\u2028\\ud7ff"
          "\\ud800\\udbff\\udc00\\udfff\\ue000\\uffff\\ud800\\udc00"
          "\\ud83d\\ude00\\udbff\\udfff\"");
}

// ---------------------------------------------------------------------------
// integers, CRC
// ---------------------------------------------------------------------------

static void test_numbers() {
    struct {
        long long v;
        const char* s;
    } cases[] = {{0, "0"},
                 {-1, "-1"},
                 {7, "7"},
                 {-10, "-10"},
                 {1234567890123LL, "1234567890123"},
                 {9223372036854775807LL, "9223372036854775807"},
                 {-9223372036854775807LL - 1, "-9223372036854775808"}};
    for (auto& c : cases) {
        std::string out;
        claimio::append_int(out, c.v);
        CHECK(out == c.s);
    }
    std::string out;
    claimio::append_uint(out, 18446744073709551615ULL);
    CHECK(out == "18446744073709551615");

    CHECK(claimio::crc32("", 0) == 0u);
    CHECK(claimio::crc32("123456789", 9) == 0xcbf43926u);
    // every length through the 4-byte and tail loops, at every alignment
    std::string buf(64, '\0');
    for (size_t i = 0; i < buf.size(); ++i) buf[i] = static_cast<char>(i * 37 + 1);
    for (size_t off = 0; off < 4; ++off)
        for (size_t n = 0; n + off <= buf.size(); ++n) {
            uint32_t bytewise = 0xffffffffu;
            for (size_t i = 0; i < n; ++i) {
                bytewise ^= static_cast<unsigned char>(buf[off + i]);
                for (int k = 0; k < 8; ++k)
                    bytewise = (bytewise & 1) ? 0xedb88320u ^ (bytewise >> 1)
                                              : bytewise >> 1;
            }
            CHECK(claimio::crc32(buf.data() + off, n) == (bytewise ^ 0xffffffffu));
        }
}

// ---------------------------------------------------------------------------
// emitters: {"a":[],"b":{},"c":[1,[2,[]],{"d":{}}],"e":{"f":[{}]}}
// ---------------------------------------------------------------------------

static void key(claimio::Emitter& e, size_t i, const char* k) {
    e.item(i);
    claimio::append_escaped(e.out(), reinterpret_cast<const uint8_t*>(k),
                            std::strlen(k));
    e.colon();
}

static std::string emit_sample(int indent) {
    claimio::Emitter e(indent);
    e.open('{', 4);
    key(e, 0, "a");
    e.open('[', 0);
    e.close(']', 0);
    key(e, 1, "b");
    e.open('{', 0);
    e.close('}', 0);
    key(e, 2, "c");
    e.open('[', 3);
    e.item(0);
    claimio::append_int(e.out(), 1);
    e.item(1);
    e.open('[', 2);
    e.item(0);
    claimio::append_int(e.out(), 2);
    e.item(1);
    e.open('[', 0);
    e.close(']', 0);
    e.close(']', 2);
    e.item(2);
    e.open('{', 1);
    key(e, 0, "d");
    e.open('{', 0);
    e.close('}', 0);
    e.close('}', 1);
    e.close(']', 3);
    key(e, 3, "e");
    e.open('{', 1);
    key(e, 0, "f");
    e.open('[', 1);
    e.item(0);
    e.open('{', 0);
    e.close('}', 0);
    e.close(']', 1);
    e.close('}', 1);
    e.close('}', 4);
    return e.out();
}

static void test_emitters() {
    CHECK(emit_sample(-1) ==
          "{\"a\":[],\"b\":{},\"c\":[1,[2,[]],{\"d\":{}}],\"e\":{\"f\":[{}]}}");
    // json.dumps(sample, indent=2, sort_keys=True)
    CHECK(emit_sample(2) ==
          "{\n"
          "  \"a\": [],\n"
          "  \"b\": {},\n"
          "  \"c\": [\n"
          "    1,\n"
          "    [\n"
          "      2,\n"
          "      []\n"
          "    ],\n"
          "    {\n"
          "      \"d\": {}\n"
          "    }\n"
          "  ],\n"
          "  \"e\": {\n"
          "    \"f\": [\n"
          "      {}\n"
          "    ]\n"
          "  }\n"
          "}");
    // indent=0: newlines, no spaces
    CHECK(emit_sample(0) ==
          "{\n\"a\": [],\n\"b\": {},\n\"c\": [\n1,\n[\n2,\n[]\n],\n{\n\"d\": "
          "{}\n}\n],\n\"e\": {\n\"f\": [\n{}\n]\n}\n}");
    claimio::Emitter empty_list(2), empty_dict(-1);
    empty_list.open('[', 0);
    empty_list.close(']', 0);
    empty_dict.open('{', 0);
    empty_dict.close('}', 0);
    CHECK(empty_list.out() == "[]");
    CHECK(empty_dict.out() == "{}");
}

// ---------------------------------------------------------------------------
// file I/O
// ---------------------------------------------------------------------------

static int count_entries(const std::string& dir, const char* prefix) {
    DIR* d = ::opendir(dir.c_str());
    if (!d) return -1;
    int n = 0;
    while (dirent* ent = ::readdir(d))
        if (std::strncmp(ent->d_name, prefix, std::strlen(prefix)) == 0) ++n;
    ::closedir(d);
    return n;
}

static int g_write_calls = 0;

// at most 7 bytes per call, EINTR on every third call
static ssize_t stingy_write(int fd, const void* p, size_t n) {
    if (++g_write_calls % 3 == 0) {
        errno = EINTR;
        return -1;
    }
    return ::write(fd, p, n < 7 ? n : 7);
}

static ssize_t failing_write(int fd, const void* p, size_t n) {
    if (++g_write_calls > 2) {
        errno = ENOSPC;
        return -1;
    }
    return ::write(fd, p, n < 5 ? n : 5);
}

static void test_files() {
    const char* base = std::getenv("TMPDIR");
    std::string tmpl = std::string(base && *base ? base : "/tmp") + "/claimio-selftest-XXXXXX";
    std::vector<char> tbuf(tmpl.begin(), tmpl.end());
    tbuf.push_back('\0');
    CHECK(::mkdtemp(tbuf.data()) != nullptr);
    const std::string dir = tbuf.data();
    const std::string tmp = dir + "/.tmp-1-0", path = dir + "/out.json";
    const char* failed = nullptr;
    std::string back;

    // success, durable and not; the second replaces the first
    for (int durable = 0; durable < 2; ++durable) {
        std::string data = durable ? "{\"durable\":true}" : "{}";
        CHECK(claimio::write_replace(tmp.c_str(), path.c_str(), data.data(),
                                     data.size(), durable != 0, &failed) == 0);
        CHECK(claimio::read_file(path.c_str(), back) == 0);
        CHECK(back == data);
        CHECK(count_entries(dir, ".tmp-") == 0);
    }

    // larger than read_file's buffer, and empty
    std::string big(100000, 'x');
    for (size_t i = 0; i < big.size(); ++i) big[i] = static_cast<char>('a' + i % 26);
    CHECK(claimio::write_replace(tmp.c_str(), path.c_str(), big.data(),
                                 big.size(), false, &failed) == 0);
    CHECK(claimio::read_file(path.c_str(), back) == 0);
    CHECK(back == big);
    CHECK(claimio::write_replace(tmp.c_str(), path.c_str(), "", 0, false,
                                 &failed) == 0);
    CHECK(claimio::read_file(path.c_str(), back) == 0);
    CHECK(back.empty());

    // short writes and EINTR: everything still lands, in order
    g_write_calls = 0;
    CHECK(claimio::write_replace(tmp.c_str(), path.c_str(), big.data(), 1000,
                                 false, &failed, stingy_write) == 0);
    CHECK(g_write_calls > 1000 / 7);
    CHECK(claimio::read_file(path.c_str(), back) == 0);
    CHECK(back == big.substr(0, 1000));

    // a write error: errno reported against tmp, tmp removed, target kept
    g_write_calls = 0;
    CHECK(claimio::write_replace(tmp.c_str(), path.c_str(), big.data(), 100,
                                 false, &failed, failing_write) == ENOSPC);
    CHECK(failed == tmp.c_str());
    CHECK(count_entries(dir, ".tmp-") == 0);
    CHECK(claimio::read_file(path.c_str(), back) == 0);
    CHECK(back == big.substr(0, 1000));

    // rename onto a non-empty directory fails; tmp is cleaned up
    const std::string sub = dir + "/busy";
    CHECK(::mkdir(sub.c_str(), 0755) == 0);
    CHECK(claimio::write_replace(tmp.c_str(), (sub + "/f").c_str(), "x", 1,
                                 false, &failed) == 0);
    const std::string tmp2 = dir + "/.tmp-1-1";
    int err = claimio::write_replace(tmp2.c_str(), sub.c_str(), "y", 1, false,
                                     &failed);
    CHECK(err == EISDIR || err == ENOTEMPTY || err == EEXIST);
    CHECK(failed == sub.c_str());
    CHECK(count_entries(dir, ".tmp-") == 0);

    // tmp already present (O_EXCL) and parent missing (ENOENT)
    CHECK(claimio::write_replace(path.c_str(), (dir + "/other").c_str(), "z",
                                 1, false, &failed) == EEXIST);
    CHECK(claimio::read_file(path.c_str(), back) == 0);  // not unlinked
    const std::string gone = dir + "/gone/.tmp-1-2";
    CHECK(claimio::write_replace(gone.c_str(), (dir + "/gone/f").c_str(), "z",
                                 1, true, &failed) == ENOENT);
    CHECK(failed == gone.c_str());
    CHECK(claimio::read_file((dir + "/gone/f").c_str(), back) == ENOENT);

    ::unlink((sub + "/f").c_str());
    ::rmdir(sub.c_str());
    ::unlink(path.c_str());
    CHECK(::rmdir(dir.c_str()) == 0);
}

int main() {
    test_escaper();
    test_numbers();
    test_emitters();
    test_files();
    if (g_failures) {
        std::fprintf(stderr, "claimio_selftest: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::puts("claimio_selftest: OK");
    return 0;
}

// Python-free core of the _claimio extension: JSON string escaping, the
// compact/indented emitters, integer formatting, CRC32 and the atomic
// tmp+rename file write. claimio.cpp walks Python objects and feeds this;
// claimio_selftest.cpp drives it stand-alone under the sanitizers, so this
// header must never include Python.h.
//
// The emitters reproduce CPython's json.dumps byte for byte in the two
// shapes the driver persists:
//   compact   json.dumps(o, sort_keys=True, separators=(",", ":"))
//   indented  json.dumps(o, sort_keys=True, indent=N)
// (ensure_ascii stays at its default, True). Key sorting is the caller's
// job: the emitter writes members in the order it is handed them.
#pragma once

#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include <fcntl.h>
#include <stdio.h>
#include <sys/types.h>
#include <unistd.h>

namespace claimio {

// ---------------------------------------------------------------------------
// string escaping (json.encoder.py_encode_basestring_ascii semantics)
// ---------------------------------------------------------------------------

inline void append_u16_escape(std::string& out, uint32_t v) {
    static const char hex[] = "0123456789abcdef";
    char buf[6] = {'\\', 'u', hex[(v >> 12) & 0xf], hex[(v >> 8) & 0xf],
                   hex[(v >> 4) & 0xf], hex[v & 0xf]};
    out.append(buf, 6);
}

// One code point. Plain is ' '..'~' minus the quote and the backslash;
// DEL (0x7f) is escaped like every other code point outside that range,
// as json.dumps does. Lone surrogates (0xD800-0xDFFF) go out as they stand;
// astral code points become a surrogate pair.
inline void append_escaped_cp(std::string& out, uint32_t c) {
    if (c >= 0x20 && c <= 0x7e && c != '"' && c != '\\') {
        out.push_back(static_cast<char>(c));
        return;
    }
    switch (c) {
        case '"': out.append("\\\"", 2); return;
        case '\\': out.append("\\\\", 2); return;
        case '\n': out.append("\\n", 2); return;
        case '\r': out.append("\\r", 2); return;
        case '\t': out.append("\\t", 2); return;
        case '\b': out.append("\\b", 2); return;
        case '\f': out.append("\\f", 2); return;
        default: break;
    }
    if (c >= 0x10000) {
        uint32_t v = c - 0x10000;
        append_u16_escape(out, 0xd800 | ((v >> 10) & 0x3ff));
        append_u16_escape(out, 0xdc00 | (v & 0x3ff));
    } else {
        append_u16_escape(out, c);
    }
}

// A whole string of fixed-width code units (CharT = uint8_t/uint16_t/
// uint32_t: Latin-1, UCS-2 or UCS-4 storage), with the surrounding quotes.
template <typename CharT>
inline void append_escaped(std::string& out, const CharT* s, size_t n) {
    out.push_back('"');
    size_t i = 0;
    while (i < n) {
        // copy a run of plain characters in one append
        size_t j = i;
        if (sizeof(CharT) == 1) {
            while (j < n) {
                uint32_t c = s[j];
                if (c < 0x20 || c > 0x7e || c == '"' || c == '\\') break;
                ++j;
            }
            if (j > i) {
                out.append(reinterpret_cast<const char*>(s) + i, j - i);
                i = j;
                continue;
            }
        }
        append_escaped_cp(out, static_cast<uint32_t>(s[i]));
        ++i;
    }
    out.push_back('"');
}

// ---------------------------------------------------------------------------
// integers
// ---------------------------------------------------------------------------

inline void append_int(std::string& out, long long v) {
    char buf[24];
    char* p = buf + sizeof(buf);
    // negate in unsigned arithmetic: -LLONG_MIN overflows a long long
    unsigned long long u = v < 0 ? 0ULL - static_cast<unsigned long long>(v)
                                 : static_cast<unsigned long long>(v);
    do {
        *--p = static_cast<char>('0' + u % 10);
        u /= 10;
    } while (u);
    if (v < 0) *--p = '-';
    out.append(p, static_cast<size_t>(buf + sizeof(buf) - p));
}

inline void append_uint(std::string& out, unsigned long long u) {
    char buf[24];
    char* p = buf + sizeof(buf);
    do {
        *--p = static_cast<char>('0' + u % 10);
        u /= 10;
    } while (u);
    out.append(p, static_cast<size_t>(buf + sizeof(buf) - p));
}

// ---------------------------------------------------------------------------
// container framing
// ---------------------------------------------------------------------------

// Writes brackets, separators and indentation around values the caller
// appends to out() itself. indent < 0 selects the compact form.
//
//   e.open('{', n);                       // n = member count
//   for each member i: e.item(i); <key>; e.colon(); <value>;
//   e.close('}', n);
class Emitter {
  public:
    explicit Emitter(int indent) : indent_(indent), depth_(0) {}

    std::string& out() { return out_; }
    bool compact() const { return indent_ < 0; }

    void open(char bracket, size_t n) {
        out_.push_back(bracket);
        if (n) ++depth_;
    }
    // before member/element number i (0-based) of a non-empty container
    void item(size_t i) {
        if (i) out_.push_back(',');
        if (indent_ >= 0) newline();
    }
    void colon() {
        if (indent_ >= 0)
            out_.append(": ", 2);
        else
            out_.push_back(':');
    }
    void close(char bracket, size_t n) {
        if (n) {
            --depth_;
            if (indent_ >= 0) newline();
        }
        out_.push_back(bracket);
    }

  private:
    void newline() {
        out_.push_back('\n');
        out_.append(static_cast<size_t>(indent_) * depth_, ' ');
    }
    std::string out_;
    int indent_;
    size_t depth_;
};

// ---------------------------------------------------------------------------
// CRC32 (IEEE 802.3, the polynomial zlib.crc32 uses), slicing-by-4
// ---------------------------------------------------------------------------

struct Crc32Table {
    uint32_t t[4][256];
    Crc32Table() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int s = 1; s < 4; ++s)
                t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xff];
    }
};

inline uint32_t crc32(const void* data, size_t n) {
    static const Crc32Table tab;
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint32_t c = 0xffffffffu;
    while (n >= 4) {
        c ^= static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 |
             static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
        c = tab.t[3][c & 0xff] ^ tab.t[2][(c >> 8) & 0xff] ^
            tab.t[1][(c >> 16) & 0xff] ^ tab.t[0][c >> 24];
        p += 4;
        n -= 4;
    }
    while (n--) c = tab.t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

// ---------------------------------------------------------------------------
// file I/O
// ---------------------------------------------------------------------------

typedef ssize_t (*write_fn_t)(int, const void*, size_t);

// Write all n bytes, resuming after EINTR and short writes. Returns 0 or
// the errno of the failing write. write_fn is a seam for the self-test.
inline int write_all(int fd, const char* data, size_t n,
                     write_fn_t write_fn = ::write) {
    while (n) {
        ssize_t w = write_fn(fd, data, n);
        if (w < 0) {
            if (errno == EINTR) continue;
            return errno;
        }
        if (w == 0) return EIO;  // no progress on a regular file
        data += w;
        n -= static_cast<size_t>(w);
    }
    return 0;
}

// tmp (O_EXCL) + write + optional fsync + close + rename(tmp, path).
// Returns 0, or the errno of the first failing step with *failed set to
// the file name that step acted on (tmp, or path for the rename); tmp is
// unlinked on every failure after it was created.
inline int write_replace(const char* tmp, const char* path, const char* data,
                         size_t n, bool durable, const char** failed,
                         write_fn_t write_fn = ::write) {
    *failed = tmp;
    int fd;
    do {
        fd = ::open(tmp, O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0644);
    } while (fd < 0 && errno == EINTR);
    if (fd < 0) return errno;
    int err = write_all(fd, data, n, write_fn);
    if (!err && durable) {
        int r;
        do {
            r = ::fsync(fd);
        } while (r < 0 && errno == EINTR);
        if (r < 0) err = errno;
    }
    // close() is not retried on EINTR: on Linux the descriptor is gone
    if (::close(fd) < 0 && !err && errno != EINTR) err = errno;
    if (!err && ::rename(tmp, path) < 0) {
        err = errno;
        *failed = path;
    }
    if (err) ::unlink(tmp);
    return err;
}

// Whole-file read. Returns 0 and fills out, or the errno (ENOENT for a
// missing file, which callers treat as "absent", not as a failure).
inline int read_file(const char* path, std::string& out) {
    int fd;
    do {
        fd = ::open(path, O_RDONLY | O_CLOEXEC);
    } while (fd < 0 && errno == EINTR);
    if (fd < 0) return errno;
    out.clear();
    char buf[8192];
    int err = 0;
    for (;;) {
        ssize_t r = ::read(fd, buf, sizeof(buf));
        if (r < 0) {
            if (errno == EINTR) continue;
            err = errno;
            break;
        }
        if (r == 0) break;
        out.append(buf, static_cast<size_t>(r));
    }
    ::close(fd);
    return err;
}

}  // namespace claimio

// _claimio: native claim persistence for the prepare hot path.
//
// A fresh prepare persists two small JSON files (the claim CDI spec and the
// checksummed checkpoint). In Python that is a dataclasses.asdict deep copy,
// three json.dumps passes (one of them through the pure-Python indenting
// encoder) and a dozen os.* wrappers that each drop and retake the GIL.
// Here it is one walk over the live objects per file and one GIL-free
// syscall sequence per write.
//
//   encode(obj, indent)            bytes == json.dumps(obj, sort_keys=True,
//                                  separators=(",", ":")) for indent None,
//                                  json.dumps(obj, indent=indent,
//                                  sort_keys=True) otherwise
//   encode_checkpoint(claim, ver)  {"checksum":crc32(v1),"v1":...,"version":ver}
//   write_replace(tmp, path, data, durable)   atomic tmp+rename, GIL released
//   read_or_none(path)             file bytes, or None when it does not exist
//
// Anything json.dumps would render differently from the subset implemented
// here (floats, non-str keys, sets, arbitrary objects) raises TypeError; the
// Python callers then use the stock encoder, so bytes on disk never change.
//
// The Python-free part lives in claimio_core.hpp (sanitizer self-test:
// claimio_selftest.cpp).

#include <pybind11/pybind11.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "claimio_core.hpp"

namespace py = pybind11;

namespace {

// Nesting bound: a reference cycle must end in an exception, not in a
// stack overflow. Deeper (legitimate) data goes to the Python encoder.
constexpr int kMaxDepth = 200;

struct DcField {
    PyObject* name;       // strong ref, lives as long as the process
    std::string key;      // the name as an escaped JSON string
};

// dataclass type -> its fields sorted by name (code point order). The type
// is kept alive so its address cannot be reused by another class.
std::unordered_map<PyTypeObject*, std::vector<DcField>> g_dataclasses;

bool type_error(const char* what, PyObject* o) {
    PyErr_Format(PyExc_TypeError, "_claimio: %s (%.200s)", what,
                 Py_TYPE(o)->tp_name);
    return false;
}

bool append_str(std::string& out, PyObject* s) {
#if PY_VERSION_HEX < 0x030C0000
    if (PyUnicode_READY(s) < 0) return false;
#endif
    const void* data = PyUnicode_DATA(s);
    size_t n = static_cast<size_t>(PyUnicode_GET_LENGTH(s));
    switch (PyUnicode_KIND(s)) {
        case PyUnicode_1BYTE_KIND:
            claimio::append_escaped(out, static_cast<const uint8_t*>(data), n);
            return true;
        case PyUnicode_2BYTE_KIND:
            claimio::append_escaped(out, static_cast<const uint16_t*>(data), n);
            return true;
        case PyUnicode_4BYTE_KIND:
            claimio::append_escaped(out, static_cast<const uint32_t*>(data), n);
            return true;
        default:
            return type_error("unsupported str storage", s);
    }
}

// Field list of a dataclass type as dataclasses.asdict sees it, or nullptr
// (no Python error set) when tp is not a dataclass.
const std::vector<DcField>* dataclass_fields(PyTypeObject* tp, bool* failed) {
    *failed = false;
    auto it = g_dataclasses.find(tp);
    if (it != g_dataclasses.end()) return &it->second;
    PyObject* tpo = reinterpret_cast<PyObject*>(tp);
    int has = PyObject_HasAttrString(tpo, "__dataclass_fields__");
    if (has <= 0) return nullptr;
    try {
        py::object fields =
            py::module_::import("dataclasses").attr("fields")(py::handle(tpo));
        std::vector<py::object> names;
        for (py::handle f : fields) {
            py::object name = f.attr("name");
            if (!PyUnicode_Check(name.ptr())) return nullptr;
            names.push_back(std::move(name));
        }
        std::sort(names.begin(), names.end(),
                  [](const py::object& a, const py::object& b) {
                      return PyUnicode_Compare(a.ptr(), b.ptr()) < 0;
                  });
        std::vector<DcField> out;
        for (auto& n : names) {
            DcField f;
            if (!append_str(f.key, n.ptr())) throw py::error_already_set();
            f.name = n.release().ptr();
            out.push_back(std::move(f));
        }
        Py_INCREF(tpo);
        return &g_dataclasses.emplace(tp, std::move(out)).first->second;
    } catch (py::error_already_set& e) {
        e.restore();
        *failed = true;
        return nullptr;
    }
}

bool encode_value(PyObject* o, claimio::Emitter& e, int depth);

bool encode_sequence(PyObject* o, claimio::Emitter& e, int depth) {
    const bool is_list = PyList_Check(o);
    const size_t n = static_cast<size_t>(is_list ? PyList_GET_SIZE(o)
                                                 : PyTuple_GET_SIZE(o));
    e.open('[', n);
    for (size_t i = 0; i < n; ++i) {
        // re-check the size: a list can shrink under a value's __getattr__
        if (is_list && i >= static_cast<size_t>(PyList_GET_SIZE(o))) {
            PyErr_SetString(PyExc_RuntimeError,
                            "_claimio: list changed size during encoding");
            return false;
        }
        PyObject* item = is_list ? PyList_GET_ITEM(o, i) : PyTuple_GET_ITEM(o, i);
        Py_INCREF(item);
        e.item(i);
        bool ok = encode_value(item, e, depth + 1);
        Py_DECREF(item);
        if (!ok) return false;
    }
    e.close(']', n);
    return true;
}

bool encode_dict(PyObject* o, claimio::Emitter& e, int depth) {
    std::vector<std::pair<PyObject*, PyObject*>> items;
    items.reserve(static_cast<size_t>(PyDict_Size(o)));
    PyObject *k, *v;
    Py_ssize_t pos = 0;
    while (PyDict_Next(o, &pos, &k, &v)) {
        if (!PyUnicode_Check(k)) return type_error("dict key is not a str", k);
        items.emplace_back(k, v);
    }
    // own the members while nested values are encoded
    for (auto& kv : items) {
        Py_INCREF(kv.first);
        Py_INCREF(kv.second);
    }
    std::sort(items.begin(), items.end(),
              [](const std::pair<PyObject*, PyObject*>& a,
                 const std::pair<PyObject*, PyObject*>& b) {
                  return PyUnicode_Compare(a.first, b.first) < 0;
              });
    bool ok = true;
    e.open('{', items.size());
    for (size_t i = 0; ok && i < items.size(); ++i) {
        e.item(i);
        ok = append_str(e.out(), items[i].first);
        if (ok) {
            e.colon();
            ok = encode_value(items[i].second, e, depth + 1);
        }
    }
    if (ok) e.close('}', items.size());
    for (auto& kv : items) {
        Py_DECREF(kv.first);
        Py_DECREF(kv.second);
    }
    return ok;
}

bool encode_dataclass(PyObject* o, const std::vector<DcField>& fields,
                      claimio::Emitter& e, int depth) {
    e.open('{', fields.size());
    for (size_t i = 0; i < fields.size(); ++i) {
        PyObject* v = PyObject_GetAttr(o, fields[i].name);
        if (!v) return false;
        e.item(i);
        e.out().append(fields[i].key);
        e.colon();
        bool ok = encode_value(v, e, depth + 1);
        Py_DECREF(v);
        if (!ok) return false;
    }
    e.close('}', fields.size());
    return true;
}

bool encode_value(PyObject* o, claimio::Emitter& e, int depth) {
    std::string& out = e.out();
    if (o == Py_None) {
        out.append("null", 4);
        return true;
    }
    // bool before int: True is an int subclass
    if (o == Py_True) {
        out.append("true", 4);
        return true;
    }
    if (o == Py_False) {
        out.append("false", 5);
        return true;
    }
    if (PyUnicode_Check(o)) return append_str(out, o);
    if (PyLong_Check(o)) {
        int overflow = 0;
        long long v = PyLong_AsLongLongAndOverflow(o, &overflow);
        if (!overflow) {
            if (v == -1 && PyErr_Occurred()) return false;
            claimio::append_int(out, v);
            return true;
        }
        // wider than a machine word: int.__repr__, as json does
        PyObject* s = PyLong_Type.tp_repr(o);
        if (!s) return false;
        Py_ssize_t len = 0;
        const char* utf8 = PyUnicode_AsUTF8AndSize(s, &len);
        if (utf8) out.append(utf8, static_cast<size_t>(len));
        Py_DECREF(s);
        return utf8 != nullptr;
    }
    if (depth > kMaxDepth) return type_error("nesting too deep", o);
    if (PyList_Check(o) || PyTuple_Check(o)) return encode_sequence(o, e, depth);
    if (PyDict_Check(o)) return encode_dict(o, e, depth);
    if (PyFloat_Check(o)) return type_error("float is left to json.dumps", o);
    if (!PyType_Check(o)) {
        bool failed = false;
        const std::vector<DcField>* fields = dataclass_fields(Py_TYPE(o), &failed);
        if (failed) return false;
        if (fields) return encode_dataclass(o, *fields, e, depth);
    }
    return type_error("unsupported type", o);
}

int parse_indent(const py::object& indent) {
    if (indent.is_none()) return -1;
    if (!PyLong_Check(indent.ptr()))
        throw py::type_error("_claimio: indent must be an int or None");
    long v = PyLong_AsLong(indent.ptr());
    if (v == -1 && PyErr_Occurred()) throw py::error_already_set();
    // json: ' ' * indent, so a negative indent is an empty one
    return v < 0 ? 0 : static_cast<int>(std::min<long>(v, 1 << 16));
}

py::bytes encode(const py::object& obj, const py::object& indent) {
    claimio::Emitter e(parse_indent(indent));
    e.out().reserve(1024);
    if (!encode_value(obj.ptr(), e, 0)) throw py::error_already_set();
    return py::bytes(e.out());
}

py::bytes encode_checkpoint(const py::object& claim, long long version) {
    claimio::Emitter e(-1);
    std::string& out = e.out();
    out.reserve(1024);
    // fixed-width slot for the head, filled in once the CRC is known and
    // right-aligned against the payload so the result is one contiguous run
    static const char kHead[] = "{\"checksum\":";
    static const char kMid[] = ",\"v1\":";
    const size_t slot = sizeof(kHead) - 1 + 10 + sizeof(kMid) - 1;
    out.assign(slot, ' ');
    if (!encode_value(claim.ptr(), e, 0)) throw py::error_already_set();
    const uint32_t crc = claimio::crc32(out.data() + slot, out.size() - slot);
    std::string head(kHead);
    claimio::append_uint(head, crc);
    head.append(kMid);
    const size_t start = slot - head.size();
    out.replace(start, head.size(), head);
    out.append(",\"version\":");
    claimio::append_int(out, version);
    out.push_back('}');
    return py::bytes(out.data() + start, out.size() - start);
}

// str / bytes / os.PathLike -> bytes in the filesystem encoding
py::object fs_path(const py::object& p) {
    PyObject* b = nullptr;
    if (!PyUnicode_FSConverter(p.ptr(), &b)) throw py::error_already_set();
    return py::reinterpret_steal<py::object>(b);
}

[[noreturn]] void raise_oserror(int err, const py::object& filename) {
    errno = err;
    PyErr_SetFromErrnoWithFilenameObject(PyExc_OSError, filename.ptr());
    throw py::error_already_set();
}

void write_replace(const py::object& tmp, const py::object& path,
                   const py::bytes& data, bool durable) {
    py::object tmp_b = fs_path(tmp), path_b = fs_path(path);
    const char* tmp_c = PyBytes_AS_STRING(tmp_b.ptr());
    const char* path_c = PyBytes_AS_STRING(path_b.ptr());
    const char* buf = PyBytes_AS_STRING(data.ptr());
    const size_t n = static_cast<size_t>(PyBytes_GET_SIZE(data.ptr()));
    const char* failed = nullptr;
    int err;
    {
        py::gil_scoped_release nogil;
        err = claimio::write_replace(tmp_c, path_c, buf, n, durable, &failed);
    }
    if (err) raise_oserror(err, failed == path_c ? path : tmp);
}

py::object read_or_none(const py::object& path) {
    py::object path_b = fs_path(path);
    const char* path_c = PyBytes_AS_STRING(path_b.ptr());
    std::string out;
    int err;
    {
        py::gil_scoped_release nogil;
        err = claimio::read_file(path_c, out);
    }
    if (err == ENOENT) return py::none();
    if (err) raise_oserror(err, path);
    return py::bytes(out);
}

}  // namespace

PYBIND11_MODULE(_claimio, m) {
    m.doc() = "native claim persistence: JSON encode, checksum, atomic write";
    m.def("encode", &encode, py::arg("obj"), py::arg("indent") = py::none());
    m.def("encode_checkpoint", &encode_checkpoint, py::arg("claim"),
          py::arg("version"));
    m.def("write_replace", &write_replace, py::arg("tmp"), py::arg("path"),
          py::arg("data"), py::arg("durable"));
    m.def("read_or_none", &read_or_none, py::arg("path"));
}

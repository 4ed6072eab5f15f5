// Host-side parsing and validation of stage artefacts: the PLY reader of hmsg_load / hmsg_read_ply and the offset check of
// hmsg_restore_stage.  No HIP in here: tests/host_c/stage_files_asan.cpp compiles this header alone under the host sanitizers.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// codes of include/hmsg.h (HMSG_OK / HMSG_ERR_INVALID / HMSG_ERR_UNSUPPORTED), restated so that the header stands alone
enum { STAGE_OK = 0, STAGE_INVALID = -1, STAGE_UNSUPPORTED = -3 };

// Open3D read_point_cloud of the files this path writes (and of Open3D's own): the x / y / z of the vertex element of a binary
// little-endian file, double or float; the element's other scalar properties and the elements behind it are skipped.
//   want_points false: only *n is set (nothing behind the header is read beyond a size check).
// Returns STAGE_OK or an error code with `msg` set; `out` is [n][3].
static inline int stage_read_ply(const std::string& path, bool want_points, long long* n_out, std::vector<double>* out, std::string* msg) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        *msg = "cannot open " + path;
        return STAGE_INVALID;
    }
    struct Closer {
        FILE* f;
        ~Closer() { fclose(f); }
    } closer{f};
    long long n = -1;
    struct Prop {
        std::string type, name;
    };
    std::vector<Prop> props;
    char line[512];
    bool ok = false, first = true, in_vertex = false, binary_le = false, have_format = false;
    int n_lines = 0;
    while (fgets(line, sizeof line, f)) {
        std::string s(line);
        const bool whole = !s.empty() && s.back() == '\n';
        if (!whole && s.size() + 1 == sizeof line) {          // a header line longer than the buffer: no file of ours or Open3D's
            *msg = path + ": PLY header line too long";
            return STAGE_INVALID;
        }
        while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
        if (first) {
            if (s != "ply") break;
            first = false;
            continue;
        }
        if (++n_lines > 4096) break;
        if (s.rfind("format", 0) == 0) {
            have_format = true;
            binary_le = s.rfind("format binary_little_endian", 0) == 0;
        } else if (s.rfind("element", 0) == 0) {
            in_vertex = s.rfind("element vertex", 0) == 0 && (s.size() == 14 || s[14] == ' ');
            if (in_vertex) {
                char* end = nullptr;
                const long long v = strtoll(s.c_str() + 14, &end, 10);
                if (end == s.c_str() + 14 || v < 0) {
                    *msg = path + ": bad vertex count in the PLY header";
                    return STAGE_INVALID;
                }
                n = v;
            }
        } else if (s.rfind("property", 0) == 0) {
            char t[64] = "", nm[64] = "";
            if (in_vertex && sscanf(s.c_str(), "property %63s %63s", t, nm) == 2) props.push_back(Prop{t, nm});
        } else if (s == "end_header") {
            ok = true;
            break;
        }
    }
    if (!ok || n < 0) {
        *msg = path + ": no PLY header";
        return STAGE_INVALID;
    }
    if (have_format && !binary_le) {
        *msg = path + ": only binary_little_endian PLY files are read";
        return STAGE_UNSUPPORTED;
    }
    size_t stride = 0;
    int offx[3] = {-1, -1, -1};
    bool dbl[3] = {true, true, true};
    for (auto& pr : props) {
        const std::string& t = pr.type;
        const size_t sz = (t == "double" || t == "float64")                                    ? 8
                          : (t == "float" || t == "float32" || t == "int" || t == "uint" || t == "int32" || t == "uint32") ? 4
                          : (t == "short" || t == "ushort" || t == "int16" || t == "uint16")  ? 2
                          : (t == "uchar" || t == "char" || t == "uint8" || t == "int8")      ? 1
                                                                                              : 0;
        if (!sz) {
            *msg = path + ": PLY property type " + t;
            return STAGE_UNSUPPORTED;
        }
        const bool real = t == "double" || t == "float64" || t == "float" || t == "float32";
        for (int a = 0; a < 3; ++a)
            if (pr.name == (a == 0 ? "x" : (a == 1 ? "y" : "z"))) {
                if (!real) {
                    *msg = path + ": PLY coordinate of type " + t;
                    return STAGE_UNSUPPORTED;
                }
                offx[a] = (int)stride, dbl[a] = sz == 8;
            }
        stride += sz;
    }
    if (n > 0 && (offx[0] < 0 || offx[1] < 0 || offx[2] < 0)) {
        *msg = path + ": PLY without x / y / z";
        return STAGE_INVALID;
    }
    // the header's promise against the bytes that are there -- before anything is sized by it
    const long body = ftell(f);
    if (body < 0 || fseek(f, 0, SEEK_END) != 0) {
        *msg = path + ": cannot seek";
        return STAGE_INVALID;
    }
    const long end = ftell(f);
    if (end < body || (n > 0 && (stride == 0 || (unsigned long long)n > (unsigned long long)(end - body) / stride))) {
        *msg = path + ": truncated PLY";
        return STAGE_INVALID;
    }
    *n_out = n;
    if (!want_points) return STAGE_OK;
    if (fseek(f, body, SEEK_SET) != 0) {
        *msg = path + ": cannot seek";
        return STAGE_INVALID;
    }
    out->assign((size_t)n * 3, 0.0);
    std::vector<unsigned char> rec((size_t)n * stride);
    if (n && fread(rec.data(), stride, (size_t)n, f) != (size_t)n) {
        *msg = path + ": truncated PLY";
        return STAGE_INVALID;
    }
    for (long long i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const unsigned char* q = rec.data() + (size_t)i * stride + offx[a];
            if (dbl[a]) {
                double d;
                memcpy(&d, q, 8);
                (*out)[(size_t)i * 3 + a] = d;
            } else {
                float fl;
                memcpy(&fl, q, 4);
                (*out)[(size_t)i * 3 + a] = fl;
            }
        }
    return STAGE_OK;
}

// inst_off of hmsg_restore_stage: n + 1 offsets, non-decreasing from 0 (a size-0 instance is allowed)
static inline int stage_check_offsets(const int64_t* off, int64_t n, std::string* msg) {
    if (n < 0 || !off) {
        *msg = "instance offsets missing";
        return STAGE_INVALID;
    }
    if (off[0] != 0) {
        *msg = "inst_off[0] must be 0";
        return STAGE_INVALID;
    }
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) {
            *msg = "inst_off must not decrease (instance " + std::to_string((long long)i) + ")";
            return STAGE_INVALID;
        }
    return STAGE_OK;
}

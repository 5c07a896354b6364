// apd_points.hip -- the life and the files of a points object (apd_points_t of include/apd_mi355x.h, struct apd_points of
// apd_points_host.h): the operations on the table of its arrays, the one function that makes a new object, the accessors,
// apd_points_create, apd_points_destroy, apd_points_write_ply, apd_points_write_vis and apd_points_read_ply, and compact_points: an object without some
// of its points.  Who fills one: the fusions (apd_fusion_call.hip), apd_points_average.hip, apd_points_merge.hip,
// apd_points_radius.hip (through compact_points); its visibility lists: apd_points_vis.hip.
//
// apd_points_create: the checks that make the arrays a cloud some fusion could have made (every later call relies on them: a
// view indexes the source lists, a bit of `sources` indexes a list), then one copy of each array, to host memory or to the device.
//
// apd_points_write_ply: ExportPointCloud's file (APD.cpp:214-254) of any points object, the fusion's own or an averaged one: the
// header, then the 15-byte or 27-byte records k_fusion_compact packs (apd_fusion_call.hip), packed here on the host from the
// arrays (device-resident points come down in chunks).
//
// apd_points_read_ply: the way back, and the way in of a cloud made elsewhere (a ground truth): the header parsed line by line into
// the offsets of the fields kept within a vertex record, the records read in chunks on the host, then apd_points_create.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_points_host.h"
#include "apd_sort.h"

namespace apd_fusion {

hipError_t alloc_arrays(apd_points_host::Scratch &scratch, PointArrays &p, size_t n, unsigned which)
{
    hipError_t e = hipSuccess;
    for_each_array([&](auto member, size_t bytes, unsigned bit) {
        if ((which & bit) && e == hipSuccess) {
            e = scratch.alloc(n * bytes, &(p.*member));
        }
    });
    return e;
}

void keep_arrays(apd_points_host::Scratch &scratch, const PointArrays &p)
{
    for_each_array([&](auto member, size_t, unsigned) {
        if (p.*member) {
            scratch.keep(p.*member);
        }
    });
}

bool alloc_host_arrays(PointArrays &p, size_t n)
{
    bool ok = true;
    for_each_array([&](auto member, size_t bytes, unsigned) {
        p.*member = static_cast<std::remove_reference_t<decltype(p.*member)>>(malloc(n * bytes > 0 ? n * bytes : 1));
        ok = ok && p.*member;
    });
    return ok;
}

void free_arrays(PointArrays &p, bool on_device)
{
    for_each_array([&](auto member, size_t, unsigned) {
        if (on_device) {
            hipFree(p.*member);
        } else {
            free(p.*member);
        }
    });
    p = PointArrays();
}

hipError_t copy_arrays(const PointArrays &to, const PointArrays &from, size_t n, hipMemcpyKind kind, unsigned which, size_t first)
{
    hipError_t e = hipSuccess;
    for_each_array([&](auto member, size_t bytes, unsigned bit) {
        if (!(which & bit) || e != hipSuccess) {
            return;
        }
        const uint8_t *src = reinterpret_cast<const uint8_t *>(from.*member) + first * bytes;
        if (kind == hipMemcpyHostToHost) {
            memcpy(to.*member, src, n * bytes);
        } else {
            e = hipMemcpy(to.*member, src, n * bytes, kind);
        }
    });
    return e;
}

}  // namespace apd_fusion

namespace apd_points_host {

void write_ply_header(FILE *f, long long count, bool normals)
{
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n%s"
               "property uchar diffuse_blue\nproperty uchar diffuse_green\nproperty uchar diffuse_red\nend_header\n", count,
            normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "");
}

apd_points *new_points(int device, int on_device, int num_views, const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices)
{
    apd_points *q = new apd_points();
    q->device = device;
    q->on_device = on_device ? 1 : 0;
    q->pair_offsets.assign(pair_offsets, pair_offsets + num_views + 1);
    q->pair_indices.assign(pair_indices, pair_indices + pair_offsets[num_views]);
    q->rows.assign(rows, rows + num_views);
    q->cols.assign(cols, cols + num_views);
    return q;
}

}  // namespace apd_points_host

extern "C" long long apd_points_count(apd_points_t p) { return p ? p->count : 0; }
extern "C" int apd_points_on_device(apd_points_t p) { return p ? p->on_device : 0; }
extern "C" const float *apd_points_xyz(apd_points_t p) { return p ? p->arrays.xyz : nullptr; }
extern "C" const float *apd_points_normal(apd_points_t p) { return p ? p->arrays.normal : nullptr; }
extern "C" const uint8_t *apd_points_bgr(apd_points_t p) { return p ? p->arrays.bgr : nullptr; }
extern "C" const uint8_t *apd_points_support(apd_points_t p) { return p ? p->arrays.support : nullptr; }
extern "C" const int32_t *apd_points_view(apd_points_t p) { return p ? p->arrays.view : nullptr; }
extern "C" const int32_t *apd_points_pixel(apd_points_t p) { return p ? p->arrays.pixel : nullptr; }
extern "C" const uint32_t *apd_points_sources(apd_points_t p) { return p ? p->arrays.sources : nullptr; }

namespace {

using apd_fusion::PointArrays;
using namespace apd_points_host;

std::string &err() { return apd_fusion::g_fusion_error; }

int create_hip_failed(const char *expr, hipError_t e, const char *, int)
{
    return apd::set_error(err(), APD_ERR_HIP, "apd_points_create: %s: %s", expr, hipGetErrorString(e));
}

#define CREATE_REFUSE(...) return apd::set_error(err(), APD_ERR_INVALID, "apd_points_create: " __VA_ARGS__)

// What apd_points_create refuses, before anything is allocated
int check_create(long long count, const float *xyz, const float *normal, const uint8_t *bgr, const uint8_t *support, const int32_t *view,
                 const int32_t *pixel, const uint32_t *sources, int num_views, const int *rows, const int *cols, const int *pair_offsets,
                 const int *pair_indices, apd_points_t *out)
{
    if (!rows || !cols || !pair_offsets || !out) {
        CREATE_REFUSE("null argument");
    }
    if (count < 0) {
        CREATE_REFUSE("a count of %lld points", count);
    }
    if (count > 0 && !(xyz && normal && bgr && support && view && pixel && sources)) {
        CREATE_REFUSE("null argument");
    }
    if (num_views < 1) {
        CREATE_REFUSE("%d views", num_views);
    }
    for (int i = 0; i < num_views; ++i) {
        if (rows[i] <= 0 || cols[i] <= 0) {
            CREATE_REFUSE("view %d has %d x %d pixels", i, cols[i], rows[i]);
        }
        if ((long long)rows[i] * cols[i] > 0x7fffffffLL) {
            CREATE_REFUSE("view %d has %d x %d pixels, more than a pixel index holds", i, cols[i], rows[i]);
        }
    }
    if (pair_offsets[0] != 0) {
        CREATE_REFUSE("pair_offsets starts at %d, not at 0", pair_offsets[0]);
    }
    for (int i = 0; i < num_views; ++i) {
        const int len = pair_offsets[i + 1] - pair_offsets[i];
        if (pair_offsets[i + 1] < pair_offsets[i]) {
            CREATE_REFUSE("pair_offsets descends at view %d", i);
        }
        if (len > APD_MAX_IMAGES) {
            CREATE_REFUSE("view %d has %d sources, more than %d", i, len, APD_MAX_IMAGES);
        }
    }
    if (pair_offsets[num_views] > 0 && !pair_indices) {
        CREATE_REFUSE("null argument");
    }
    for (int i = 0; i < num_views; ++i) {
        for (int e = pair_offsets[i]; e < pair_offsets[i + 1]; ++e) {
            if (pair_indices[e] < 0 || pair_indices[e] >= num_views) {
                CREATE_REFUSE("source %d of view %d is view %d of %d", e - pair_offsets[i], i, pair_indices[e], num_views);
            }
            if (pair_indices[e] == i) {
                CREATE_REFUSE("view %d is its own source", i);
            }
        }
    }
    for (long long k = 0; k < count; ++k) {
        const int v = view[k];
        if (v < 0 || v >= num_views) {
            CREATE_REFUSE("point %lld is of view %d of %d", k, v, num_views);
        }
        if (pixel[k] < 0 || pixel[k] >= rows[v] * cols[v]) {
            CREATE_REFUSE("point %lld is pixel %d of view %d, which has %d", k, pixel[k], v, rows[v] * cols[v]);
        }
        const int len = pair_offsets[v + 1] - pair_offsets[v];
        if (len < 32 && (sources[k] >> len) != 0) {
            CREATE_REFUSE("point %lld names sources 0x%x, its view %d has %d", k, sources[k], v, len);
        }
        if (__builtin_popcount(sources[k]) != (int)support[k]) {
            CREATE_REFUSE("point %lld names %d sources and has a support of %d", k, __builtin_popcount(sources[k]), (int)support[k]);
        }
    }
    return APD_OK;
}

#undef CREATE_REFUSE

// one copy of each of the caller's arrays where the object lives
int create_arrays(apd_points *q, const PointArrays &from)
{
    const auto hip_failed = create_hip_failed;
    const size_t n = (size_t)q->count;
    PointArrays a;
    if (q->on_device) {
        Scratch scratch;  // of the arrays until every copy is made
        HIP_TRY(hipSetDevice(q->device));
        HIP_TRY(alloc_arrays(scratch, a, n));
        HIP_TRY(copy_arrays(a, from, n, hipMemcpyHostToDevice));
        keep_arrays(scratch, a);
    } else if (!alloc_host_arrays(a, n)) {
        free_arrays(a, false);
        return apd::set_error(err(), APD_ERR_HIP, "apd_points_create: out of host memory");
    } else {
        copy_arrays(a, from, n, hipMemcpyHostToHost);
    }
    q->arrays = a;
    return APD_OK;
}

}  // namespace

extern "C" int apd_points_create(int device, int on_device, long long count, const float *xyz, const float *normal, const uint8_t *bgr,
                                 const uint8_t *support, const int32_t *view, const int32_t *pixel, const uint32_t *sources, int num_views,
                                 const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices, apd_points_t *out)
{
    err().clear();
    if (const int rc = check_create(count, xyz, normal, bgr, support, view, pixel, sources, num_views, rows, cols, pair_offsets, pair_indices, out);
        rc != APD_OK) {
        return rc;
    }
    apd_points *q = new_points(device, on_device, num_views, rows, cols, pair_offsets, pair_indices);
    q->count = count;
    if (count > 0) {
        DeviceScope scope(q->on_device != 0);
        // the caller's arrays, in the order of PointArrays: read only
        const PointArrays from = {const_cast<float *>(xyz),      const_cast<float *>(normal),  const_cast<uint8_t *>(bgr),     const_cast<uint8_t *>(support),
                                  const_cast<int32_t *>(view), const_cast<int32_t *>(pixel), const_cast<uint32_t *>(sources)};
        if (const int rc = create_arrays(q, from); rc != APD_OK) {
            apd_points_destroy(q);  // it has no arrays yet; keeps the message
            return rc;
        }
    }
    *out = q;
    return APD_OK;
}

extern "C" int apd_points_destroy(apd_points_t p)
{
    if (!p) {
        return APD_OK;
    }
    DeviceScope scope(p->on_device != 0);
    if (p->on_device) {
        hipSetDevice(p->device);
        hipFree(p->vis_offsets);
        hipFree(p->vis_views);
    } else {
        free(p->vis_offsets);
        free(p->vis_views);
    }
    apd_fusion::free_arrays(p->arrays, p->on_device != 0);
    delete p;
    return APD_OK;
}

extern "C" int apd_points_write_ply(apd_points_t p, const char *path, int with_normals)
{
    err().clear();
    if (!p || !path) {
        return apd::set_error(err(), APD_ERR_INVALID, "apd_points_write_ply: null argument");
    }
    const size_t n = (size_t)p->count;
    const size_t floats = with_normals ? 6 : 3, record = 4 * floats + 3;
    const size_t kChunk = 1u << 20;  // points per download and per fwrite
    const PointArrays &a = p->arrays;
    std::vector<float> xyz, normal;
    std::vector<uint8_t> bgr, packed;
    DeviceScope scope(p->on_device && n > 0);
    if (p->on_device && n > 0) {
        const hipError_t e = hipSetDevice(p->device);
        if (e != hipSuccess) {
            return apd::set_error(err(), APD_ERR_HIP, "apd_points_write_ply: hipSetDevice: %s", hipGetErrorString(e));
        }
        xyz.resize(3 * std::min(n, kChunk));
        normal.resize(with_normals ? xyz.size() : 0);
        bgr.resize(xyz.size());
    }
    FILE *f = fopen(path, "wb");
    if (!f) {
        err() = std::string("apd_points_write_ply: cannot write ") + path;  // no length limit: not through set_error
        return APD_ERR_IO;
    }
    write_ply_header(f, p->count, with_normals != 0);
    bool ok = true;
    for (size_t k0 = 0; k0 < n && ok; k0 += kChunk) {
        const size_t m = std::min(n - k0, kChunk);
        const float *cx = a.xyz + 3 * k0, *cn = a.normal + 3 * k0;
        const uint8_t *cb = a.bgr + 3 * k0;
        if (p->on_device) {
            PointArrays chunk;
            chunk.xyz = xyz.data();
            chunk.normal = normal.data();
            chunk.bgr = bgr.data();
            const unsigned which = apd_fusion::kXyz | apd_fusion::kBgr | (with_normals ? apd_fusion::kNormal : 0u);
            const hipError_t e = copy_arrays(chunk, a, m, hipMemcpyDeviceToHost, which, k0);
            if (e != hipSuccess) {
                fclose(f);
                return apd::set_error(err(), APD_ERR_HIP, "apd_points_write_ply: download of the points: %s", hipGetErrorString(e));
            }
            cx = xyz.data();
            cn = normal.data();
            cb = bgr.data();
        }
        packed.resize(m * record);
        for (size_t k = 0; k < m; ++k) {  // little endian floats, as the host's memcpy writes them
            uint8_t *rec = packed.data() + k * record;
            memcpy(rec, cx + 3 * k, 12);
            if (with_normals) {
                memcpy(rec + 12, cn + 3 * k, 12);
            }
            memcpy(rec + 4 * floats, cb + 3 * k, 3);
        }
        ok = fwrite(packed.data(), 1, packed.size(), f) == packed.size();
    }
    if (fclose(f) != 0 || !ok) {
        err() = std::string("apd_points_write_ply: short write to ") + path;
        return APD_ERR_IO;
    }
    return APD_OK;
}

extern "C" int apd_points_write_vis(apd_points_t p, const char *path)
{
    err().clear();
    if (!p || !path) {
        return apd::set_error(err(), APD_ERR_INVALID, "apd_points_write_vis: null argument");
    }
    const long long *offsets = nullptr;
    const int32_t *views = nullptr;
    if (const int rc = apd_points_visibility(p, &offsets, &views); rc != APD_OK) {
        return rc;
    }
    const size_t n = (size_t)p->count;
    std::vector<long long> host_offsets;
    std::vector<int32_t> host_views;
    if (p->on_device) {  // one download of each array
        DeviceScope scope(true);
        host_offsets.resize(n + 1);
        hipError_t e = hipSetDevice(p->device);
        e = e != hipSuccess ? e : hipMemcpy(host_offsets.data(), offsets, (n + 1) * sizeof(long long), hipMemcpyDeviceToHost);
        if (e == hipSuccess && host_offsets[n] > 0) {
            host_views.resize((size_t)host_offsets[n]);
            e = hipMemcpy(host_views.data(), views, host_views.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
        }
        if (e != hipSuccess) {
            return apd::set_error(err(), APD_ERR_HIP, "apd_points_write_vis: download of the lists: %s", hipGetErrorString(e));
        }
        offsets = host_offsets.data();
        views = host_views.data();
    }
    FILE *f = fopen(path, "wb");
    if (!f) {
        err() = std::string("apd_points_write_vis: cannot write ") + path;
        return APD_ERR_IO;
    }
    // uint64 number of points, then per point uint32 n and n x uint32 view index, little endian like every file of the project
    const uint64_t count = (uint64_t)n;
    bool ok = fwrite(&count, 8, 1, f) == 1;
    std::vector<uint32_t> chunk;
    const size_t kChunk = 1u << 16;  // points per fwrite
    for (size_t k0 = 0; k0 < n && ok; k0 += kChunk) {
        const size_t k1 = std::min(n, k0 + kChunk);
        chunk.clear();
        for (size_t k = k0; k < k1; ++k) {
            chunk.push_back((uint32_t)(offsets[k + 1] - offsets[k]));
            for (long long e = offsets[k]; e < offsets[k + 1]; ++e) {
                chunk.push_back((uint32_t)views[e]);
            }
        }
        ok = fwrite(chunk.data(), 4, chunk.size(), f) == chunk.size();
    }
    if (fclose(f) != 0 || !ok) {
        err() = std::string("apd_points_write_vis: short write to ") + path;
        return APD_ERR_IO;
    }
    return APD_OK;
}

// --------------------------------------------------------------------------------------------------------------------
// apd_points_read_ply
// --------------------------------------------------------------------------------------------------------------------

namespace {

// A scalar type of a PLY header: its size in bytes, 0: not one; *real32 / *byte8: it is `float` / `uchar`
size_t ply_scalar(const std::string &type, bool *real32, bool *byte8)
{
    static const struct {
        const char *name;
        size_t size;
    } kinds[] = {{"char", 1}, {"uchar", 1}, {"int8", 1}, {"uint8", 1}, {"short", 2}, {"ushort", 2}, {"int16", 2}, {"uint16", 2},
                 {"int", 4},  {"uint", 4},  {"int32", 4}, {"uint32", 4}, {"float", 4}, {"float32", 4}, {"double", 8}, {"float64", 8}};
    *real32 = type == "float" || type == "float32";
    *byte8 = type == "uchar" || type == "uint8";
    for (const auto &k : kinds) {
        if (type == k.name) {
            return k.size;
        }
    }
    return 0;
}

std::vector<std::string> words_of(const std::string &line)
{
    std::vector<std::string> words;
    size_t at = 0;
    while (at < line.size()) {
        const size_t from = line.find_first_not_of(" \t\r", at);
        if (from == std::string::npos) {
            break;
        }
        const size_t to = line.find_first_of(" \t\r", from);
        words.push_back(line.substr(from, to == std::string::npos ? to : to - from));
        at = to == std::string::npos ? line.size() : to;
    }
    return words;
}

// Where the fields apd_points_read_ply keeps stand in a vertex record; -1: not in the file
struct PlyLayout {
    long long count = -1;  // of `element vertex`; -1: none seen
    size_t record = 0;
    int xyz[3] = {-1, -1, -1}, normal[3] = {-1, -1, -1}, bgr[3] = {-1, -1, -1};
};

int refuse_ply(int code, const char *path, const std::string &why)
{
    err() = std::string("apd_points_read_ply: ") + path + ": " + why;  // no length limit: not through set_error
    return code;
}

// The header of the file at f, up to and including end_header
int read_ply_header(FILE *f, const char *path, PlyLayout &layout)
{
    std::string line;
    bool first = true, format = false, in_vertex = false, after_vertex = false;
    for (;;) {
        line.clear();
        int c = 0;
        while ((c = fgetc(f)) != EOF && c != '\n') {
            line.push_back((char)c);
            if (line.size() > 4096) {
                return refuse_ply(APD_ERR_INVALID, path, "a header line of more than 4096 bytes");
            }
        }
        if (c == EOF) {
            return first && line != "ply" ? refuse_ply(APD_ERR_INVALID, path, "not a PLY file") : refuse_ply(APD_ERR_IO, path, "the file ends inside the header");
        }
        const std::vector<std::string> w = words_of(line);
        if (first) {
            if (w.size() != 1 || w[0] != "ply") {
                return refuse_ply(APD_ERR_INVALID, path, "not a PLY file");
            }
            first = false;
            continue;
        }
        if (w.empty() || w[0] == "comment" || w[0] == "obj_info") {
            continue;
        }
        if (w[0] == "end_header") {
            break;
        }
        if (w[0] == "format") {
            if (w.size() != 3 || w[1] != "binary_little_endian" || w[2] != "1.0") {
                return refuse_ply(APD_ERR_INVALID, path, "format " + (w.size() > 1 ? w[1] : std::string("?")) + ", not binary_little_endian 1.0");
            }
            format = true;
        } else if (w[0] == "element") {
            if (w.size() != 3) {
                return refuse_ply(APD_ERR_INVALID, path, "a malformed element line");
            }
            in_vertex = w[1] == "vertex";
            if (in_vertex) {
                char *end = nullptr;
                const long long n = strtoll(w[2].c_str(), &end, 10);
                if (layout.count >= 0 || w[2].find_first_not_of("0123456789") != std::string::npos || *end != '\0' || w[2].size() > 18) {
                    return refuse_ply(APD_ERR_INVALID, path, "element vertex " + w[2] + ", not one count of vertices");
                }
                layout.count = n;
            } else if (layout.count < 0) {
                return refuse_ply(APD_ERR_INVALID, path, "element " + w[1] + " before element vertex");
            } else {
                after_vertex = true;
            }
        } else if (w[0] == "property") {
            if (after_vertex) {
                continue;  // of an element that is not read
            }
            if (!in_vertex) {
                return refuse_ply(APD_ERR_INVALID, path, "a property before any element");
            }
            if (w.size() >= 2 && w[1] == "list") {
                return refuse_ply(APD_ERR_INVALID, path, "a list property in element vertex");
            }
            bool real32 = false, byte8 = false;
            const size_t size = w.size() == 3 ? ply_scalar(w[1], &real32, &byte8) : 0;
            if (size == 0) {
                return refuse_ply(APD_ERR_INVALID, path, "a malformed property line: " + line);
            }
            static const char *const coordinate[3] = {"x", "y", "z"}, *const normal[3] = {"nx", "ny", "nz"}, *const colour[3] = {"blue", "green", "red"};
            for (int a = 0; a < 3; ++a) {
                if (w[2] == coordinate[a]) {
                    if (!real32) {
                        return refuse_ply(APD_ERR_INVALID, path, "coordinate " + w[2] + " is " + w[1] + ", not float");
                    }
                    layout.xyz[a] = (int)layout.record;
                } else if (w[2] == normal[a] && real32) {
                    layout.normal[a] = (int)layout.record;
                } else if ((w[2] == colour[a] || w[2] == std::string("diffuse_") + colour[a]) && byte8) {
                    layout.bgr[a] = (int)layout.record;
                }
            }
            layout.record += size;
            if (layout.record > 65536) {
                return refuse_ply(APD_ERR_INVALID, path, "a vertex record of more than 65536 bytes");
            }
        } else {
            return refuse_ply(APD_ERR_INVALID, path, "an unknown header line: " + line);
        }
    }
    if (!format) {
        return refuse_ply(APD_ERR_INVALID, path, "no format line");
    }
    if (layout.count < 0) {
        return refuse_ply(APD_ERR_INVALID, path, "no element vertex");
    }
    for (int a = 0; a < 3; ++a) {
        if (layout.xyz[a] < 0) {
            return refuse_ply(APD_ERR_INVALID, path, std::string("no float coordinate ") + "xyz"[a] + " in element vertex");
        }
    }
    return APD_OK;
}

}  // namespace

extern "C" int apd_points_read_ply(const char *path, int device, int on_device, apd_points_t *out)
{
    err().clear();
    if (!path || !out) {
        return apd::set_error(err(), APD_ERR_INVALID, "apd_points_read_ply: null argument");
    }
    FILE *f = fopen(path, "rb");
    if (!f) {
        return refuse_ply(APD_ERR_IO, path, "cannot read the file");
    }
    PlyLayout layout;
    if (const int rc = read_ply_header(f, path, layout); rc != APD_OK) {
        fclose(f);
        return rc;
    }
    const size_t n = (size_t)layout.count;
    const bool normals = layout.normal[0] >= 0 && layout.normal[1] >= 0 && layout.normal[2] >= 0;
    const bool colours = layout.bgr[0] >= 0 && layout.bgr[1] >= 0 && layout.bgr[2] >= 0;
    std::vector<float> xyz, normal;
    std::vector<uint8_t> bgr, records;
    const size_t kChunk = std::max<size_t>(((size_t)1 << 24) / layout.record, 1);  // records per fread: 16 MiB of them
    bool ok = true;
    for (size_t k0 = 0; k0 < n && ok; k0 += kChunk) {
        const size_t m = std::min(n - k0, kChunk);
        records.resize(m * layout.record);
        ok = fread(records.data(), 1, records.size(), f) == records.size();
        xyz.resize(3 * (k0 + (ok ? m : 0)));  // grows with what the file holds, not with what its header says
        normal.resize(xyz.size(), 0.0f);
        bgr.resize(xyz.size(), 0);
        for (size_t k = 0; k < m && ok; ++k) {  // little endian floats, as the host's memcpy reads them
            const uint8_t *rec = records.data() + k * layout.record;
            for (int a = 0; a < 3; ++a) {
                memcpy(&xyz[3 * (k0 + k) + a], rec + layout.xyz[a], 4);
                if (normals) {
                    memcpy(&normal[3 * (k0 + k) + a], rec + layout.normal[a], 4);
                }
                if (colours) {
                    bgr[3 * (k0 + k) + a] = rec[layout.bgr[a]];
                }
            }
        }
    }
    fclose(f);
    if (!ok) {
        return refuse_ply(APD_ERR_IO, path, "the file ends before its " + std::to_string(layout.count) + " vertices of " + std::to_string(layout.record) +
                                                " bytes do");
    }
    // one view of 1 x 1 without sources: every point is its pixel 0 and has no support
    const std::vector<uint8_t> support(n, 0);
    const std::vector<int32_t> zeros(n, 0);
    const std::vector<uint32_t> sources(n, 0);
    const int rows[1] = {1}, cols[1] = {1}, pair_offsets[2] = {0, 0};
    const int rc = apd_points_create(device, on_device, layout.count, xyz.data(), normal.data(), bgr.data(), support.data(), zeros.data(), zeros.data(),
                                     sources.data(), 1, rows, cols, pair_offsets, nullptr, out);
    if (rc != APD_OK) {
        err() = std::string("apd_points_read_ply: ") + path + ": " + err();
    }
    return rc;
}

// --------------------------------------------------------------------------------------------------------------------
// compact_points
// --------------------------------------------------------------------------------------------------------------------

namespace {

// `width` elements per point: those of the kept points k go to point at[k] (the kept points before k)
template <typename T>
__global__ __launch_bounds__(256) void k_compact_array(const T *__restrict__ in, int width, const uint32_t *__restrict__ keep,
                                                        const uint64_t *__restrict__ at, size_t n, T *__restrict__ out)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n && keep[k]) {
        const size_t to = (size_t)at[k];
        for (int c = 0; c < width; ++c) {
            out[to * width + c] = in[k * width + c];
        }
    }
}

// length[k]: entries of the list of point k if it is kept, else 0
__global__ __launch_bounds__(256) void k_kept_list_lengths(const long long *__restrict__ offsets, const uint32_t *__restrict__ keep, size_t n,
                                                            uint32_t *__restrict__ length)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        length[k] = keep[k] ? (uint32_t)(offsets[k + 1] - offsets[k]) : 0u;
    }
}

// The list of kept point k starts at entry_at[k] (the kept entries before it) and belongs to point at[k]; [kept] = all of them
__global__ __launch_bounds__(256) void k_compact_lists(const long long *__restrict__ offsets, const int32_t *__restrict__ views,
                                                        const uint32_t *__restrict__ keep, const uint64_t *__restrict__ at,
                                                        const uint64_t *__restrict__ entry_at, size_t n, long long *__restrict__ out_offsets,
                                                        int32_t *__restrict__ out_views)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) {
        return;
    }
    if (keep[k]) {
        out_offsets[at[k]] = (long long)entry_at[k];
        int32_t *to = out_views + entry_at[k];
        for (long long e = offsets[k]; e < offsets[k + 1]; ++e) {
            *to++ = views[e];
        }
    }
    if (k == 0) {
        out_offsets[at[n]] = (long long)entry_at[n];
    }
}

}  // namespace

int apd_points_host::compact_points(const char *who, const apd_points *p, const apd_fusion::PointArrays &in, const uint32_t *keep,
                                    apd_points *result)
{
    using apd_fusion::PointArrays;
    const auto hip_failed = [who](const char *expr, hipError_t e, const char *, int) {  // what HIP_TRY returns here
        return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_HIP, "%s: %s: %s", who, expr, hipGetErrorString(e));
    };
    const auto no_host_memory = [who] { return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_HIP, "%s: out of host memory", who); };
    const size_t n = (size_t)p->count;
    const dim3 blocks((unsigned)((n + 255) / 256));  // n < 2^31: fits
    Scratch scratch;
    // p's lists where p lives, before anything of the result exists: a merged object's are all it has
    const long long *offsets = nullptr;
    const int32_t *views = nullptr;
    if (p->merged) {
        if (const int rc = apd_points_visibility(const_cast<apd_points *>(p), &offsets, &views); rc != APD_OK) {
            return rc;
        }
    }
    uint64_t *at = nullptr;
    HIP_TRY(scratch.alloc((n + 1) * 8, &at));
    HIP_TRY(apd_sort::exclusive_scan(keep, at, n));
    uint64_t kept = 0;
    HIP_TRY(hipMemcpy(&kept, at + n, 8, hipMemcpyDeviceToHost));
    const size_t m = (size_t)kept;
    result->merged = p->merged;
    result->count = (long long)m;
    if (m == 0) {  // an object without points
        return APD_OK;
    }
    PointArrays out;
    HIP_TRY(alloc_arrays(scratch, out, m));
    apd_fusion::for_each_array([&](auto member, size_t bytes, unsigned) {
        if (bytes % 4 == 0) {
            hipLaunchKernelGGL(k_compact_array<uint32_t>, blocks, dim3(256), 0, 0, reinterpret_cast<const uint32_t *>(in.*member), (int)(bytes / 4), keep,
                               (const uint64_t *)at, n, reinterpret_cast<uint32_t *>(out.*member));
        } else {
            hipLaunchKernelGGL(k_compact_array<uint8_t>, blocks, dim3(256), 0, 0, reinterpret_cast<const uint8_t *>(in.*member), (int)bytes, keep,
                               (const uint64_t *)at, n, reinterpret_cast<uint8_t *>(out.*member));
        }
    });
    HIP_TRY(hipGetLastError());
    long long *out_offsets = nullptr;
    int32_t *out_views = nullptr;
    size_t entries = 0;
    if (p->merged) {
        if (!p->on_device) {
            const size_t total = (size_t)offsets[n];
            HIP_TRY(scratch.upload(offsets, (n + 1) * sizeof(long long), &offsets));
            HIP_TRY(scratch.upload(views, total * sizeof(int32_t), &views));
        }
        uint32_t *length = nullptr;
        uint64_t *entry_at = nullptr;
        HIP_TRY(scratch.alloc(n * 4, &length));
        HIP_TRY(scratch.alloc((n + 1) * 8, &entry_at));
        hipLaunchKernelGGL(k_kept_list_lengths, blocks, dim3(256), 0, 0, offsets, keep, n, length);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(length, entry_at, n));
        uint64_t total = 0;
        HIP_TRY(hipMemcpy(&total, entry_at + n, 8, hipMemcpyDeviceToHost));
        entries = (size_t)total;
        HIP_TRY(scratch.alloc((m + 1) * sizeof(long long), &out_offsets));
        HIP_TRY(scratch.alloc(entries * sizeof(int32_t), &out_views));
        hipLaunchKernelGGL(k_compact_lists, blocks, dim3(256), 0, 0, offsets, views, keep, (const uint64_t *)at, (const uint64_t *)entry_at, n, out_offsets,
                           out_views);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    if (p->on_device) {
        keep_arrays(scratch, out);
        result->arrays = out;
        if (p->merged) {
            scratch.keep(out_offsets);
            scratch.keep(out_views);
            result->vis_offsets = out_offsets;
            result->vis_views = out_views;
        }
        return APD_OK;
    }
    // host memory: freed with `result` by the caller if a download fails
    if (!alloc_host_arrays(result->arrays, m)) {
        return no_host_memory();
    }
    HIP_TRY(copy_arrays(result->arrays, out, m, hipMemcpyDeviceToHost));
    if (p->merged) {
        result->vis_offsets = static_cast<long long *>(malloc((m + 1) * sizeof(long long)));
        result->vis_views = static_cast<int32_t *>(malloc(entries > 0 ? entries * sizeof(int32_t) : sizeof(int32_t)));
        if (!result->vis_offsets || !result->vis_views) {
            return no_host_memory();
        }
        HIP_TRY(hipMemcpy(result->vis_offsets, out_offsets, (m + 1) * sizeof(long long), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(result->vis_views, out_views, entries * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return APD_OK;
}

// mesh_io.cpp -- surface mesh files (include/frog_host.h: frog_mesh_*), chosen by extension as the reference's ReadPolyData and
// WritePolyData choose them (tools/MeshTransform.cxx:62-64).  Points and polygons only: normals, texture coordinates, colours
// and every other attribute are read past and not carried.
// The readers take the whole file into memory and walk it with a cursor that cannot pass its end: a truncated or malformed
// file is refused with a status and a message (frog_mesh_last_error), whatever its header promises.  This file depends on
// nothing but the C++ library, so tests/mesh_driver.cpp compiles it on its own under the sanitizers.
#include "frog_host.h"

#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

thread_local std::string g_error;

struct Mesh {
    std::vector<float> xyz;
    std::vector<uint32_t> ptr{ 0 }, idx;
    size_t points() const { return xyz.size() / 3; }
    void face_end() { ptr.push_back((uint32_t)idx.size()); }
};

struct Refusal { std::string what; };
[[noreturn]] void refuse(const std::string &what) { throw Refusal{ what }; }

// The file's bytes, never read past `end`.  A NUL follows the last byte so that strtod and strtoll stop there.
struct Cursor {
    const char *p, *end;
    size_t left() const { return (size_t)(end - p); }
    bool done() const { return p >= end; }
    void skip_space() { while (p < end && isspace((unsigned char)*p)) p++; }
    // the next blank-separated token; empty at the end of the file
    std::string token()
    {
        skip_space();
        const char *b = p;
        while (p < end && !isspace((unsigned char)*p)) p++;
        return std::string(b, p);
    }
    // the rest of the current line, without its end; the cursor moves past the line end
    std::string line()
    {
        const char *b = p;
        while (p < end && *p != '\n') p++;
        const char *e = p;
        if (p < end) p++;
        while (e > b && (e[-1] == '\r')) e--;
        return std::string(b, e);
    }
    // past the end of the line a header keyword stood on: binary data starts right after it
    void end_of_line()
    {
        while (p < end && *p != '\n' && isspace((unsigned char)*p)) p++;
        if (p < end && *p == '\n') p++;
    }
    const unsigned char *bytes(size_t n, const char *what)
    {
        if (n > left()) refuse(std::string("the file ends inside ") + what);
        const unsigned char *b = (const unsigned char *)p;
        p += n;
        return b;
    }
};

double to_double(const std::string &t, const char *what)
{
    if (t.empty()) refuse(std::string("the file ends where ") + what + " is expected");
    char *e = nullptr;
    const double v = strtod(t.c_str(), &e);
    if (e == t.c_str() || *e) refuse(std::string("'") + t.substr(0, 32) + "' is not a number (" + what + ")");
    return v;
}

long long to_integer(const std::string &t, const char *what)
{
    if (t.empty()) refuse(std::string("the file ends where ") + what + " is expected");
    char *e = nullptr;
    errno = 0;
    const long long v = strtoll(t.c_str(), &e, 10);
    if (e == t.c_str() || *e || errno) refuse(std::string("'") + t.substr(0, 32) + "' is not an integer (" + what + ")");
    return v;
}

// a count a header declares: every counted item takes at least `least` bytes of what is left of the file
size_t to_count(const std::string &t, const Cursor &c, size_t least, const char *what)
{
    const long long v = to_integer(t, what);
    if (v < 0 || (unsigned long long)v > c.left() / least + 1) refuse(std::string(what) + ": " + t + " do not fit the file");
    return (size_t)v;
}

void add_index(Mesh &m, long long i, const char *what)
{
    if (i < 0 || i > 0xFFFFFFFEll) refuse(std::string(what) + ": index " + std::to_string(i) + " out of range");
    m.idx.push_back((uint32_t)i);
}

std::string lower(std::string s)
{
    for (char &ch : s) ch = (char)tolower((unsigned char)ch);
    return s;
}

template <class T> T load(const unsigned char *b, bool big_endian)
{
    unsigned char r[sizeof(T)];
    for (size_t k = 0; k < sizeof(T); k++) r[k] = big_endian ? b[sizeof(T) - 1 - k] : b[k];      // the host is little-endian
    T v;
    memcpy(&v, r, sizeof(T));
    return v;
}

// ---- Wavefront OBJ -----------------------------------------------------------------------------------------------------------

void read_obj(Cursor c, Mesh &m)
{
    while (!c.done()) {
        const std::string text = c.line();
        Cursor l{ text.data(), text.data() + text.size() };
        const std::string key = l.token();
        if (key == "v") {
            for (int k = 0; k < 3; k++) m.xyz.push_back((float)to_double(l.token(), "a vertex coordinate"));
        } else if (key == "f") {
            size_t n = 0;
            for (std::string t = l.token(); !t.empty(); t = l.token(), n++) {
                long long i = to_integer(t.substr(0, t.find('/')), "a face index");     // i, i/t, i//n, i/t/n
                if (i == 0) refuse("OBJ face index 0");
                i = i < 0 ? (long long)m.points() + i : i - 1;
                add_index(m, i, "OBJ face");
            }
            if (n < 3) refuse("an OBJ face with fewer than three vertices");
            m.face_end();
        }
    }
}

// ---- PLY -----------------------------------------------------------------------------------------------------------------------

enum PlyType { P_I8, P_U8, P_I16, P_U16, P_I32, P_U32, P_F32, P_F64, P_NONE };

PlyType ply_type(const std::string &t)
{
    static const char *names[2][8] = { { "char", "uchar", "short", "ushort", "int", "uint", "float", "double" },
                                       { "int8", "uint8", "int16", "uint16", "int32", "uint32", "float32", "float64" } };
    for (int s = 0; s < 2; s++)
        for (int k = 0; k < 8; k++)
            if (t == names[s][k]) return (PlyType)k;
    refuse("PLY: unknown type '" + t.substr(0, 32) + "'");
}

size_t ply_size(PlyType t) { static const size_t s[8] = { 1, 1, 2, 2, 4, 4, 4, 8 }; return s[t]; }

struct PlyProperty { std::string name; PlyType type = P_NONE, count_type = P_NONE; };     // count_type != P_NONE: a list
struct PlyElement { std::string name; size_t count = 0; std::vector<PlyProperty> properties; };

double ply_value(Cursor &c, PlyType t, bool ascii)
{
    if (ascii) return to_double(c.token(), "a PLY value");
    const unsigned char *b = c.bytes(ply_size(t), "a PLY element");
    switch (t) {
    case P_I8: return load<int8_t>(b, false);
    case P_U8: return load<uint8_t>(b, false);
    case P_I16: return load<int16_t>(b, false);
    case P_U16: return load<uint16_t>(b, false);
    case P_I32: return load<int32_t>(b, false);
    case P_U32: return load<uint32_t>(b, false);
    case P_F32: return load<float>(b, false);
    default: return load<double>(b, false);
    }
}

void read_ply(Cursor c, Mesh &m)
{
    if (c.line() != "ply") refuse("not a PLY file");
    bool ascii = false, format = false;
    std::vector<PlyElement> elements;
    for (;;) {
        if (c.done()) refuse("the file ends inside the PLY header");
        const std::string text = c.line();
        Cursor l{ text.data(), text.data() + text.size() };
        const std::string key = l.token();
        if (key == "end_header") break;
        if (key == "format") {
            const std::string f = l.token();
            if (f != "ascii" && f != "binary_little_endian") refuse("PLY format '" + f.substr(0, 32) + "' is not read");
            ascii = f == "ascii"; format = true;
        } else if (key == "element") {
            PlyElement e;
            e.name = l.token();
            e.count = to_count(l.token(), c, 1, "PLY element count");
            elements.push_back(e);
        } else if (key == "property") {
            if (elements.empty()) refuse("PLY: a property before the first element");
            PlyProperty p;
            std::string t = l.token();
            if (t == "list") {
                p.count_type = ply_type(l.token());
                if (p.count_type >= P_F32) refuse("PLY: a list count has an integer type");
                t = l.token();
            }
            p.type = ply_type(t);
            p.name = l.token();
            elements.back().properties.push_back(p);
        }
    }
    if (!format) refuse("PLY: no format line");
    for (const PlyElement &e : elements) {
        const bool vertex = e.name == "vertex", face = e.name == "face";
        int axis[3] = { -1, -1, -1 };
        for (size_t k = 0; k < e.properties.size(); k++)
            for (int a = 0; a < 3; a++)
                if (vertex && e.properties[k].count_type == P_NONE && e.properties[k].name == std::string(1, "xyz"[a])) axis[a] = (int)k;
        if (vertex && (axis[0] < 0 || axis[1] < 0 || axis[2] < 0)) refuse("PLY: the vertex element has no x, y, z");
        if (!ascii && e.properties.empty() && e.count) refuse("PLY: an element without properties");
        for (size_t n = 0; n < e.count; n++) {
            float p[3] = { 0, 0, 0 };
            for (size_t k = 0; k < e.properties.size(); k++) {
                const PlyProperty &q = e.properties[k];
                if (q.count_type == P_NONE) {
                    const double v = ply_value(c, q.type, ascii);
                    for (int a = 0; a < 3; a++)
                        if (axis[a] == (int)k) p[a] = (float)v;
                    continue;
                }
                const double count = ply_value(c, q.count_type, ascii);
                const bool keep = face && (q.name == "vertex_indices" || q.name == "vertex_index");
                if (!(count >= 0) || count > (double)c.left() / (ascii ? 2.0 : (double)ply_size(q.type)) + 1) refuse("PLY: a list longer than the file");
                if (keep && q.type >= P_F32) refuse("PLY: face indices have an integer type");
                for (size_t i = 0; i < (size_t)count; i++) {
                    const double v = ply_value(c, q.type, ascii);
                    if (keep) add_index(m, v == floor(v) ? (long long)v : -1, "PLY face");
                }
                if (keep) m.face_end();
            }
            if (vertex) m.xyz.insert(m.xyz.end(), p, p + 3);
        }
    }
}

// ---- STL -----------------------------------------------------------------------------------------------------------------------

struct PointKey {
    uint32_t b[3];
    bool operator==(const PointKey &o) const { return b[0] == o.b[0] && b[1] == o.b[1] && b[2] == o.b[2]; }
};
struct PointHash {
    size_t operator()(const PointKey &k) const { return ((size_t)k.b[0] * 0x9E3779B1u) ^ ((size_t)k.b[1] * 0x85EBCA77u) ^ ((size_t)k.b[2] * 0xC2B2AE3Du) ^ ((size_t)k.b[1] << 32); }
};

// points with equal bit patterns are one point, numbered in first-occurrence order
struct PointMerger {
    Mesh &m;
    std::unordered_map<PointKey, uint32_t, PointHash> seen;
    void add(const float p[3])
    {
        PointKey k;
        memcpy(k.b, p, sizeof k.b);
        auto it = seen.find(k);
        if (it == seen.end()) {
            it = seen.emplace(k, (uint32_t)m.points()).first;
            m.xyz.insert(m.xyz.end(), p, p + 3);
        }
        m.idx.push_back(it->second);
    }
};

void read_stl(Cursor c, Mesh &m)
{
    PointMerger merge{ m, {} };
    const size_t size = c.left();
    if (size >= 84) {
        const uint32_t n = load<uint32_t>((const unsigned char *)c.p + 80, false);
        if (84 + 50 * (size_t)n == size) {
            c.bytes(84, "the STL header");
            for (uint32_t f = 0; f < n; f++) {
                const unsigned char *b = c.bytes(50, "an STL facet");
                for (int v = 0; v < 3; v++) {
                    float p[3];
                    for (int k = 0; k < 3; k++) p[k] = load<float>(b + 12 + 12 * v + 4 * k, false);
                    merge.add(p);
                }
                m.face_end();
            }
            return;
        }
    }
    if (c.token() != "solid") refuse("neither a binary STL of the size its count gives nor an ASCII STL");
    c.line();
    bool closed = false;
    while (!closed) {
        const std::string key = c.token();
        if (key.empty()) refuse("the file ends before endsolid");
        if (key == "endsolid") { closed = true; break; }
        if (key != "facet") refuse("ASCII STL: '" + key.substr(0, 32) + "' where a facet is expected");
        c.line();                                                       // normal nx ny nz
        if (c.token() != "outer" || c.token() != "loop") refuse("ASCII STL: outer loop expected");
        size_t n = 0;
        for (std::string t = c.token(); t != "endloop"; t = c.token(), n++) {
            if (t != "vertex") refuse("ASCII STL: vertex or endloop expected");
            float p[3];
            for (int k = 0; k < 3; k++) p[k] = (float)to_double(c.token(), "an STL coordinate");
            merge.add(p);
        }
        if (n < 3) refuse("ASCII STL: a loop with fewer than three vertices");
        m.face_end();
        if (c.token() != "endfacet") refuse("ASCII STL: endfacet expected");
    }
}

// ---- legacy VTK POLYDATA -------------------------------------------------------------------------------------------------------

// n values of a legacy VTK array: ASCII tokens, or big-endian binary of the given width (is_float: float / double, else signed
// integers of 4 or 8 bytes)
std::vector<double> vtk_values(Cursor &c, size_t n, bool binary, size_t width, bool is_float, const char *what)
{
    std::vector<double> v;
    if (binary) {
        c.end_of_line();
        if (n > c.left() / width) refuse(std::string("the file ends inside ") + what);
        const unsigned char *b = c.bytes(n * width, what);
        v.resize(n);
        for (size_t i = 0; i < n; i++, b += width)
            v[i] = is_float ? (width == 4 ? (double)load<float>(b, true) : load<double>(b, true))
                            : (width == 4 ? (double)load<int32_t>(b, true) : (double)load<int64_t>(b, true));
    } else {
        if (n > c.left() / 2 + 1) refuse(std::string("the file ends inside ") + what);
        v.resize(n);
        for (size_t i = 0; i < n; i++) v[i] = to_double(c.token(), what);
    }
    return v;
}

size_t vtk_int_width(const std::string &type)
{
    const std::string t = lower(type);
    if (t == "vtktypeint64" || t == "long" || t == "vtkidtype") return 8;
    if (t == "vtktypeint32" || t == "int") return 4;
    refuse("VTK: cell array type '" + type.substr(0, 32) + "' is not read");
}

// One cell section (POLYGONS, TRIANGLE_STRIPS, and the ones read past) in either layout: cells[i] = the point ids of cell i.
void vtk_cells(Cursor &c, bool binary, std::vector<std::vector<long long>> &cells)
{
    const size_t a = to_count(c.token(), c, 1, "VTK cell count"), b = to_count(c.token(), c, 1, "VTK cell array size");
    Cursor probe = c;
    if (lower(probe.token()) == "offsets") {            // OFFSETS type / CONNECTIVITY type: a offsets, b ids
        c = probe;
        const size_t wo = vtk_int_width(c.token());
        const std::vector<double> off = vtk_values(c, a, binary, wo, false, "VTK offsets");
        if (lower(c.token()) != "connectivity") refuse("VTK: CONNECTIVITY expected");
        const size_t wc = vtk_int_width(c.token());
        const std::vector<double> ids = vtk_values(c, b, binary, wc, false, "VTK connectivity");
        for (size_t i = 0; i + 1 < a; i++) {
            if (!(off[i] >= 0 && off[i] <= off[i + 1] && off[i + 1] <= (double)b)) refuse("VTK: offsets out of order");
            cells.emplace_back();
            for (size_t k = (size_t)off[i]; k < (size_t)off[i + 1]; k++) cells.back().push_back((long long)ids[k]);
        }
    } else {                                            // classic: a cells in b integers, each cell its count then its ids
        const std::vector<double> v = vtk_values(c, b, binary, 4, false, "VTK cells");
        size_t k = 0;
        for (size_t i = 0; i < a; i++) {
            if (k >= b || !(v[k] >= 0) || v[k] > (double)(b - k - 1)) refuse("VTK: a cell longer than its section");
            const size_t n = (size_t)v[k++];
            cells.emplace_back();
            for (size_t j = 0; j < n; j++) cells.back().push_back((long long)v[k++]);
        }
    }
}

void read_vtk(Cursor c, Mesh &m)
{
    if (c.line().compare(0, 5, "# vtk") != 0) refuse("not a legacy VTK file");
    c.line();
    const std::string mode = lower(c.token());
    if (mode != "ascii" && mode != "binary") refuse("VTK: ASCII or BINARY expected");
    const bool binary = mode == "binary";
    if (lower(c.token()) != "dataset" || lower(c.token()) != "polydata") refuse("VTK: DATASET POLYDATA expected");
    bool points = false;
    for (;;) {
        const std::string key = lower(c.token());
        if (key.empty() || key == "point_data" || key == "cell_data") break;        // attributes are not carried
        if (key == "points") {
            const size_t n = to_count(c.token(), c, 3, "VTK point count");
            const std::string type = lower(c.token());
            if (type != "float" && type != "double") refuse("VTK: POINTS as float or double");
            const std::vector<double> v = vtk_values(c, 3 * n, binary, type == "float" ? 4 : 8, true, "VTK points");
            for (double x : v) m.xyz.push_back((float)x);
            points = true;
        } else if (key == "polygons" || key == "triangle_strips" || key == "vertices" || key == "lines") {
            std::vector<std::vector<long long>> cells;
            vtk_cells(c, binary, cells);
            for (const auto &cell : cells) {
                if (key == "polygons") {
                    for (long long i : cell) add_index(m, i, "VTK polygon");
                    m.face_end();
                } else if (key == "triangle_strips") {
                    for (size_t i = 0; i + 2 < cell.size(); i++) {
                        add_index(m, cell[i + (i & 1)], "VTK strip");
                        add_index(m, cell[i + 1 - (i & 1)], "VTK strip");
                        add_index(m, cell[i + 2], "VTK strip");
                        m.face_end();
                    }
                }
            }
        } else if (key == "metadata") {                     // a block of text up to an empty line
            c.line();
            while (!c.done() && !c.line().empty()) {}
        } else {
            refuse("VTK: section '" + key.substr(0, 32) + "' is not read");
        }
    }
    if (!points) refuse("VTK: no POINTS");
}

bool ends_with(const std::string &s, const char *suffix)
{
    const size_t n = strlen(suffix);
    return s.size() >= n && lower(s.substr(s.size() - n)) == suffix;
}

int check_mesh(const frog_mesh *m)
{
    if (!m || (m->n_points && !m->xyz) || !m->face_ptr || (m->n_faces && m->face_ptr[m->n_faces] && !m->face_idx)) return FROG_E_INVALID;
    if (m->face_ptr[0] != 0) return FROG_E_INVALID;
    for (uint32_t f = 0; f < m->n_faces; f++)
        if (m->face_ptr[f + 1] < m->face_ptr[f]) return FROG_E_INVALID;
    for (uint32_t k = 0; k < m->face_ptr[m->n_faces]; k++)
        if (m->face_idx[k] >= m->n_points) return FROG_E_INVALID;
    return FROG_OK;
}

struct File {
    FILE *f;
    explicit File(const char *path, const char *mode) : f(fopen(path, mode)) {}
    ~File() { if (f) fclose(f); }
    int close()
    {
        const bool bad = ferror(f) != 0;
        const int rc = fclose(f);
        f = nullptr;
        return bad || rc ? FROG_E_IO : FROG_OK;
    }
};

} // namespace

struct frog_mesh_file { Mesh mesh; };

extern "C" {

const char *frog_mesh_last_error(void) { return g_error.c_str(); }

frog_mesh_file *frog_mesh_read(const char *path, int *status)
{
    auto fail = [&](int code, const std::string &what) {
        g_error = std::string(path ? path : "(null)") + ": " + what;
        if (status) *status = code;
        return (frog_mesh_file *)nullptr;
    };
    if (!path) return fail(FROG_E_INVALID, "no path");
    const std::string name(path);
    void (*reader)(Cursor, Mesh &) = ends_with(name, ".obj") ? read_obj : ends_with(name, ".ply") ? read_ply
                                   : ends_with(name, ".stl") ? read_stl : ends_with(name, ".vtk") ? read_vtk : nullptr;
    if (!reader) return fail(FROG_E_INVALID, "a mesh is read from .obj, .ply, .stl or .vtk");
    std::vector<char> raw;
    {
        File in(path, "rb");
        if (!in.f) return fail(FROG_E_IO, "cannot open the file");
        char block[1 << 16];
        for (size_t n; (n = fread(block, 1, sizeof block, in.f)) > 0;) raw.insert(raw.end(), block, block + n);
        if (ferror(in.f)) return fail(FROG_E_IO, "cannot read the file");
    }
    raw.push_back('\0');
    frog_mesh_file *f = nullptr;
    try {
        f = new frog_mesh_file;
        reader(Cursor{ raw.data(), raw.data() + raw.size() - 1 }, f->mesh);
        Mesh &m = f->mesh;
        if (m.points() > 0xFFFFFFFEull || m.ptr.size() > 0xFFFFFFFEull || m.idx.size() > 0xFFFFFFFEull) refuse("more than 2^32 points, faces or indices");
        for (uint32_t i : m.idx)
            if (i >= m.points()) refuse("face index " + std::to_string(i) + " with " + std::to_string(m.points()) + " points");
    } catch (const Refusal &r) {
        delete f;
        return fail(FROG_E_INVALID, r.what);
    } catch (const std::bad_alloc &) {
        delete f;
        return fail(FROG_E_NOMEM, "out of host memory");
    }
    if (status) *status = FROG_OK;
    return f;
}

void frog_mesh_view(const frog_mesh_file *f, frog_mesh *out)
{
    if (!f || !out) return;
    Mesh &m = const_cast<Mesh &>(f->mesh);
    out->n_points = (uint32_t)m.points();
    out->xyz = m.xyz.data();
    out->n_faces = (uint32_t)m.ptr.size() - 1;
    out->face_ptr = m.ptr.data();
    out->face_idx = m.idx.data();
}

void frog_mesh_free(frog_mesh_file *f) { delete f; }

int frog_mesh_write(const char *path, const frog_mesh *m)
{
    auto fail = [&](int code, const std::string &what) { g_error = std::string(path ? path : "(null)") + ": " + what; return code; };
    if (!path) return fail(FROG_E_INVALID, "no path");
    if (check_mesh(m)) return fail(FROG_E_INVALID, "a mesh's face_ptr ascends from 0 and its indices lie inside the points");
    const std::string name(path);
    const bool obj = ends_with(name, ".obj"), ply = ends_with(name, ".ply"), stl = ends_with(name, ".stl"), vtk = ends_with(name, ".vtk"),
               vtp = ends_with(name, ".vtp");
    if (!(obj || ply || stl || vtk || vtp)) return fail(FROG_E_INVALID, "a mesh is written to .obj, .ply, .stl, .vtk or .vtp");
    File out(path, "wb");
    if (!out.f) return fail(FROG_E_IO, "cannot open the file for writing");
    FILE *f = out.f;
    const uint32_t np = m->n_points, nf = m->n_faces, ni = m->face_ptr[nf];
    if (obj) {
        for (uint32_t i = 0; i < np; i++) fprintf(f, "v %.9g %.9g %.9g\n", m->xyz[3 * i], m->xyz[3 * i + 1], m->xyz[3 * i + 2]);
        for (uint32_t k = 0; k < nf; k++) {
            fputc('f', f);
            for (uint32_t j = m->face_ptr[k]; j < m->face_ptr[k + 1]; j++) fprintf(f, " %u", m->face_idx[j] + 1);
            fputc('\n', f);
        }
    } else if (ply) {
        uint32_t longest = 0;
        for (uint32_t k = 0; k < nf; k++) longest = std::max(longest, m->face_ptr[k + 1] - m->face_ptr[k]);
        const bool wide = longest > 255;
        fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment libfrog_host\nelement vertex %u\nproperty float x\nproperty float y\n"
                   "property float z\nelement face %u\nproperty list %s uint vertex_indices\nend_header\n", np, nf, wide ? "uint" : "uchar");
        if (np) fwrite(m->xyz, sizeof(float), 3 * (size_t)np, f);
        for (uint32_t k = 0; k < nf; k++) {
            const uint32_t n = m->face_ptr[k + 1] - m->face_ptr[k];
            const uint8_t n8 = (uint8_t)n;
            if (wide) fwrite(&n, 4, 1, f);
            else fwrite(&n8, 1, 1, f);
            if (n) fwrite(m->face_idx + m->face_ptr[k], 4, n, f);
        }
    } else if (stl) {
        uint64_t n_tri = 0;
        for (uint32_t k = 0; k < nf; k++) n_tri += m->face_ptr[k + 1] - m->face_ptr[k] >= 3 ? m->face_ptr[k + 1] - m->face_ptr[k] - 2 : 0;
        if (n_tri > 0xFFFFFFFFull) return fail(FROG_E_INVALID, "more than 2^32 triangles");
        char header[80] = "binary STL written by libfrog_host";
        const uint32_t n32 = (uint32_t)n_tri;
        fwrite(header, 1, 80, f);
        fwrite(&n32, 4, 1, f);
        for (uint32_t k = 0; k < nf; k++) {
            const uint32_t *id = m->face_idx + m->face_ptr[k], n = m->face_ptr[k + 1] - m->face_ptr[k];
            if (n < 3) continue;
            const float *a = m->xyz + 3 * (size_t)id[0], *b = m->xyz + 3 * (size_t)id[1], *c = m->xyz + 3 * (size_t)id[2];
            const float u[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, v[3] = { c[0] - a[0], c[1] - a[1], c[2] - a[2] };
            float normal[3] = { u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0] };
            const float len = sqrtf(normal[0] * normal[0] + normal[1] * normal[1] + normal[2] * normal[2]);
            for (int q = 0; q < 3; q++) normal[q] = len > 0 && std::isfinite(len) ? normal[q] / len : 0.0f;
            for (uint32_t j = 1; j + 1 < n; j++) {              // the fan (0, j, j + 1)
                const uint16_t attribute = 0;
                fwrite(normal, 4, 3, f);
                fwrite(a, 4, 3, f);
                fwrite(m->xyz + 3 * (size_t)id[j], 4, 3, f);
                fwrite(m->xyz + 3 * (size_t)id[j + 1], 4, 3, f);
                fwrite(&attribute, 2, 1, f);
            }
        }
    } else if (vtk) {
        fprintf(f, "# vtk DataFile Version 3.0\nmesh written by libfrog_host\nASCII\nDATASET POLYDATA\nPOINTS %u float\n", np);
        for (uint32_t i = 0; i < np; i++) fprintf(f, "%.9g %.9g %.9g\n", m->xyz[3 * i], m->xyz[3 * i + 1], m->xyz[3 * i + 2]);
        fprintf(f, "POLYGONS %u %llu\n", nf, (unsigned long long)nf + ni);
        for (uint32_t k = 0; k < nf; k++) {
            fprintf(f, "%u", m->face_ptr[k + 1] - m->face_ptr[k]);
            for (uint32_t j = m->face_ptr[k]; j < m->face_ptr[k + 1]; j++) fprintf(f, " %u", m->face_idx[j]);
            fputc('\n', f);
        }
    } else {
        fprintf(f, "<?xml version=\"1.0\"?>\n<VTKFile type=\"PolyData\" version=\"0.1\" byte_order=\"LittleEndian\">\n  <PolyData>\n"
                   "    <Piece NumberOfPoints=\"%u\" NumberOfVerts=\"0\" NumberOfLines=\"0\" NumberOfStrips=\"0\" NumberOfPolys=\"%u\">\n"
                   "      <Points>\n        <DataArray type=\"Float32\" NumberOfComponents=\"3\" format=\"ascii\">\n", np, nf);
        for (uint32_t i = 0; i < np; i++) fprintf(f, "%.9g %.9g %.9g\n", m->xyz[3 * i], m->xyz[3 * i + 1], m->xyz[3 * i + 2]);
        fprintf(f, "        </DataArray>\n      </Points>\n      <Polys>\n        <DataArray type=\"Int64\" Name=\"connectivity\" format=\"ascii\">\n");
        for (uint32_t k = 0; k < nf; k++) {
            for (uint32_t j = m->face_ptr[k]; j < m->face_ptr[k + 1]; j++) fprintf(f, j == m->face_ptr[k] ? "%u" : " %u", m->face_idx[j]);
            fputc('\n', f);
        }
        fprintf(f, "        </DataArray>\n        <DataArray type=\"Int64\" Name=\"offsets\" format=\"ascii\">\n");
        for (uint32_t k = 0; k < nf; k++) fprintf(f, "%u\n", m->face_ptr[k + 1]);
        fprintf(f, "        </DataArray>\n      </Polys>\n    </Piece>\n  </PolyData>\n</VTKFile>\n");
    }
    if (out.close()) return fail(FROG_E_IO, "cannot write the file");
    return FROG_OK;
}

} // extern "C"

// Scene ingestion and device-table construction (host side, plain C++).  The culling hierarchy is pt_cull_tables.cpp.
//
// Follows the behaviour of Scene::LoadModel (scene.cpp:26-109), Triangle's constructor and SetNormal
// (triangles.h:27-44) and Factory (material.h:58-106) of the reference; the code is new.
#include "pt_scene.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>

namespace pt {

namespace {

// GLM scalar semantics used at set-up time: dot3 = x+y+z of the products (left to right),
// normalize = v * (1/sqrt(dot)), cross as in glm/detail/func_geometric.inl.
inline float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

void set_plane_from_normal(float *rec, const float *normal) {   // Triangle::SetNormal, triangles.h:40-44
    const float inv = 1.0f / std::sqrt(dot3(normal, normal));
    const float n[3] = {normal[0] * inv, normal[1] * inv, normal[2] * inv};
    rec[0] = n[0];
    rec[1] = n[1];
    rec[2] = n[2];
    rec[3] = -dot3(n, rec + 4);
}

struct ObjIndex {
    int v = -1, vt = -1, vn = -1;
};

// "a/b/c" -> indices 0 and 2, each atoi()-1 (scene.cpp:6-14,90-96); missing fields give -1.  The middle one, which the reference
// never looks at, likewise (an empty field, "a//c", gives -1 too: atoi("") is 0).
ObjIndex parse_face_group(const std::string &g) {
    ObjIndex r;
    const size_t s1 = g.find('/');
    r.v = std::atoi(g.substr(0, s1).c_str()) - 1;
    if (s1 != std::string::npos) {
        const size_t s2 = g.find('/', s1 + 1);
        r.vt = std::atoi(g.substr(s1 + 1, s2 == std::string::npos ? std::string::npos : s2 - s1 - 1).c_str()) - 1;
        if (s2 != std::string::npos) {
            const size_t s3 = g.find('/', s2 + 1);
            r.vn = std::atoi(g.substr(s2 + 1, s3 == std::string::npos ? std::string::npos : s3 - s2 - 1).c_str()) - 1;
        }
    }
    return r;
}

// The MTL reader of scene.cpp:45-71: every run of the outer loop appends one material, fields are picked out of
// a flat token stream, and the stream's eof flag (not its fail flag) ends both loops.
// map_Kd: the token after it is recorded as the material's texture file name (HostScene::map_kd) and otherwise treated as the
// reference treats it -- it goes through the dispatch as any token does, since the reference does not know the line.  Pr likewise:
// the token after it, where it is a finite number, is recorded as the material's roughness (HostScene::mat_pr).
void read_mtl(std::istream &in, std::vector<float> &mat, std::vector<std::string> &map_kd, std::vector<float> &mat_pr) {
    std::string tok = "1";
    while (!in.eof()) {
        float rec[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        std::string kd_name;
        float pr = -1.0f;
        while (!in.eof() && tok != "newmtl") in >> tok;
        in >> tok;   // the material's name; it then goes through the same dispatch as any other token
        while (!in.eof() && tok != "newmtl") {
            if (tok == "Kd") in >> rec[0] >> rec[1] >> rec[2];
            else if (tok == "Ke") in >> rec[3] >> rec[4] >> rec[5];
            else if (tok == "Ks") in >> rec[6] >> rec[7] >> rec[8];
            else if (tok == "Ns") in >> rec[9];
            const bool was_map_kd = tok == "map_Kd", was_pr = tok == "Pr";
            in >> tok;
            if (was_map_kd && !in.fail()) kd_name = tok;
            if (was_pr && !in.fail()) {
                char *end = nullptr;
                const float v = std::strtof(tok.c_str(), &end);
                if (end != tok.c_str() && *end == '\0' && std::isfinite(v)) pr = v;
            }
            if (in.fail() && !in.eof()) return;   // the reference would spin forever on a non-numeric field
        }
        mat.insert(mat.end(), rec, rec + 10);
        map_kd.push_back(kd_name);
        mat_pr.push_back(pr);
    }
}

}  // namespace

void append_triangle(HostScene &s, const float v0[3], const float v1[3], const float v2[3], const float *vn, int material, const float *toward) {
    float rec[14];
    std::memcpy(rec + 4, v0, 12);
    std::memcpy(rec + 7, v1, 12);
    std::memcpy(rec + 10, v2, 12);
    const float ab[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float ac[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const float c[3] = {ab[1] * ac[2] - ac[1] * ab[2], ab[2] * ac[0] - ac[2] * ab[0], ab[0] * ac[1] - ac[0] * ab[1]};
    set_plane_from_normal(rec, c);        // triangles.h:34
    rec[13] = std::sqrt(dot3(c, c));      // triangles.h:35
    if (vn) set_plane_from_normal(rec, vn);   // scene.cpp:102-104
    else if (toward && dot3(c, toward) < 0.0f) {   // PT_LOAD_GEOMETRIC_PLANES: the cross product, on the side the file's vn names
        const float back[3] = {-c[0], -c[1], -c[2]};
        set_plane_from_normal(rec, back);
    }
    s.tri.insert(s.tri.end(), rec, rec + 14);
    s.tri_mat.push_back(material);
}

bool load_obj(const std::string &dir, const std::string &name, HostScene &out, std::string &err, bool &io_error, bool geometric_planes) {
    io_error = false;
    std::ifstream obj(dir + name);
    if (!obj.is_open()) {
        err = "cannot open " + dir + name;
        io_error = true;
        return false;
    }
    std::vector<float> pos, nrm, tex;
    int current_material = 0;
    std::string tok;
    while (!obj.eof()) {
        obj >> tok;
        if (obj.eof()) break;
        if (obj.fail()) {
            err = "unreadable token stream in " + name;
            return false;
        }
        if (tok == "mtllib") {
            std::string mtl_name;
            obj >> mtl_name;
            std::ifstream mtl(dir + mtl_name);
            if (!mtl.is_open()) {   // the reference loops forever here
                err = "cannot open " + dir + mtl_name;
                io_error = true;
                return false;
            }
            read_mtl(mtl, out.mat, out.map_kd, out.mat_pr);
        } else if (tok == "v") {
            float p[3] = {0, 0, 0};
            obj >> p[0] >> p[1] >> p[2];
            pos.insert(pos.end(), p, p + 3);
        } else if (tok == "vt") {
            float uv[2] = {0, 0};
            obj >> uv[0] >> uv[1];
            tex.insert(tex.end(), uv, uv + 2);
        } else if (tok == "vn") {
            float n[3] = {0, 0, 0};
            obj >> n[0] >> n[1] >> n[2];
            nrm.insert(nrm.end(), n, n + 3);
        } else if (tok == "f") {
            ObjIndex idx[3];
            for (auto &g : idx) {
                std::string group;
                obj >> group;
                g = parse_face_group(group);
            }
            const int nv = static_cast<int>(pos.size() / 3), nn = static_cast<int>(nrm.size() / 3);
            for (const auto &g : idx)
                if (g.v < 0 || g.v >= nv) {
                    err = "face refers to vertex " + std::to_string(g.v + 1) + " of " + std::to_string(nv);
                    return false;
                }
            if (current_material < 0 || current_material >= out.n_mat()) {
                err = "usemtl " + std::to_string(current_material) + " with " + std::to_string(out.n_mat()) + " materials";
                return false;
            }
            for (const auto &g : idx)   // (the reference reads the first corner's only; the other two are kept for the shading normals)
                if (g.vn >= nn) {
                    err = "face refers to normal " + std::to_string(g.vn + 1) + " of " + std::to_string(nn);
                    return false;
                }
            const int nt = static_cast<int>(tex.size() / 2);
            for (const auto &g : idx)
                if (nt > 0 && g.vt >= nt) {   // (a file without vt lines: the index means nothing, as to the reference, and the corner gets (0, 0))
                    err = "face refers to texture coordinate " + std::to_string(g.vt + 1) + " of " + std::to_string(nt);
                    return false;
                }
            append_triangle(out, &pos[3 * idx[0].v], &pos[3 * idx[1].v], &pos[3 * idx[2].v],
                            idx[0].vn >= 0 && !geometric_planes ? &nrm[3 * idx[0].vn] : nullptr, current_material,
                            idx[0].vn >= 0 && geometric_planes ? &nrm[3 * idx[0].vn] : nullptr);
            for (const auto &g : idx) {   // each corner its own vn, as the file gives it; the face's stored normal without one
                const float *n = g.vn >= 0 ? &nrm[3 * g.vn] : &out.tri[out.tri.size() - 14];
                out.tri_vn.insert(out.tri_vn.end(), n, n + 3);
            }
            for (const auto &g : idx) {   // each corner its own vt; (0, 0) without one
                const bool has = g.vt >= 0 && g.vt < nt;
                out.tri_uv.push_back(has ? tex[2 * g.vt] : 0.0f);
                out.tri_uv.push_back(has ? tex[2 * g.vt + 1] : 0.0f);
            }
        } else if (tok == "usemtl") {
            obj >> current_material;   // scene.cpp:105-106: an int, used directly as the index
            if (obj.fail() && !obj.eof()) {
                err = "usemtl expects the integer index of a material (as the reference does)";
                return false;
            }
        }
        if (obj.fail() && !obj.eof()) {
            err = "malformed numeric field after '" + tok + "'";
            return false;
        }
    }
    return true;
}

void build_device_tables(const HostScene &s, DeviceTables &out) {
    const int T = s.n_tri();
    out.exact.resize(T);
    for (int i = 0; i < T; ++i) {
        const float *r = &s.tri[14 * static_cast<size_t>(i)];
        ExactRec &e = out.exact[i];
        std::memcpy(e.plane, r, 16);
        std::memcpy(e.v0, r + 4, 12);
        e.square = r[13];
        std::memcpy(e.v1, r + 7, 12);
        e.material = s.tri_mat[i];
        std::memcpy(e.v2, r + 10, 12);
        e.orig = i;
    }
    out.mats.resize(s.n_mat());
    for (int m = 0; m < s.n_mat(); ++m) {   // Factory, material.h:58-106
        const float *p = &s.mat[10 * static_cast<size_t>(m)];
        MatRec &d = out.mats[m];
        std::memset(&d, 0, sizeof d);
        std::memcpy(d.kd, p, 12);
        std::memcpy(d.ks, p + 6, 12);
        const float Ns = p[9];
        const bool ke = material_emits(p);
        const bool ks = p[6] != 0.0f || p[7] != 0.0f || p[8] != 0.0f;
        int n = 0;
        int kind[2] = {0, 0};
        float chance[2] = {0, 0};
        if (ke) {
            kind[n] = 0; chance[n] = 1.0f; ++n;
        } else {
            if (Ns != 0.0f && ks) { kind[n] = 1; chance[n] = Ns / 1000; ++n; }
            if (1 - Ns / 1000 > 0) { kind[n] = 2; chance[n] = 1 - Ns / 1000; ++n; }
        }
        d.n_lobes = n; d.kind0 = kind[0]; d.kind1 = kind[1];
        d.chance0 = chance[0]; d.chance1 = chance[1];
    }
}

}  // namespace pt

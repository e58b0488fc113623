// Host API above the C ABI (include/rustsasa_amd.hpp), part 1 of 5: the helpers shared with the reference's utils.rs
// and the radii - the embedded ProtOr table, FreeSASA-format configs, element van-der-Waals radii.  (reader.cpp reads
// structures, prepare.cpp selects atoms, writer.cpp prints results, files_mode.cpp runs levels and directory mode.)
// No SASA arithmetic happens in the host layer: per-atom values and the sequential f32 segment sums come from the GPU
// (rsasa_calculate_sasa_batch).
#include "host_internal.h"

#include <fstream>
#include <sstream>

namespace rustsasa {

using detail::ProtorFlat;

// utils.rs:24-33
std::int64_t serialize_chain_id(const std::string &s)
{
    std::int64_t result = 0;
    for (unsigned char c : s)
        if (std::isalpha(c)) result = result * 10 + ((std::int64_t)std::toupper(c) - 64);
    return result;
}

std::uint64_t fnv_hash_altloc_serial(const std::string &alt, std::size_t serial)
{
    return detail::fnv_id({alt.data(), alt.size()}, serial);
}

// consts.rs:7-16
bool is_polar_residue(const std::string &name)
{
    static const char *polar[] = {"SER", "THR", "CYS", "ASN", "GLN", "TYR"};
    for (const char *p : polar)
        if (name == p) return true;
    return false;
}

struct ProtorEntry { const char *residue, *atom; float radius; };
static const ProtorEntry kProtor[] = {
#include "protor_table.inc"
};

static const RadiiConfig &protor_map()
{
    static const RadiiConfig m = [] {
        RadiiConfig t;
        for (const auto &e : kProtor) t[e.residue][e.atom] = e.radius;
        return t;
    }();
    return m;
}

ProtorFlat::ProtorFlat()
{
    for (auto &k : key) k = 0;  // (no packed name pair is 0)
    for (const auto &e : kProtor) {
        std::uint64_t k;
        if (!pack(e.residue, std::strlen(e.residue), e.atom, std::strlen(e.atom), &k)) continue;
        unsigned s = slot(k);
        while (key[s] != 0 && key[s] != k) s = (s + 1) & (kSize - 1);
        key[s] = k;
        radius[s] = e.radius;
    }
}

const ProtorFlat &detail::protor_flat()
{
    static const ProtorFlat flat;
    return flat;
}

bool get_protor_radius(const std::string &residue, const std::string &atom, float *out)
{
    if (detail::protor_flat().find({residue.data(), residue.size()}, {atom.data(), atom.size()}, out)) return true;
    if (residue.size() <= 4 && atom.size() <= 4 && !residue.empty() && !atom.empty()) return false;  // packs, not there
    const auto &m = protor_map();  // (names the flat table cannot hold: the general lookup)
    auto r = m.find(residue);
    if (r == m.end()) return false;
    auto a = r->second.find(atom);
    if (a == r->second.end()) return false;
    *out = a->second;
    return true;
}

// consts.rs:31-81
RadiiConfig parse_radii_config(const std::string &content)
{
    std::unordered_map<std::string, float> types;
    RadiiConfig atoms;
    bool in_types = false, in_atoms = false;
    std::istringstream is(content);
    std::string raw;
    while (std::getline(is, raw)) {
        std::string line = detail::trim(raw);
        if (line.empty() || line[0] == '#' || line.rfind("name:", 0) == 0) continue;
        if (line == "types:") { in_types = true; in_atoms = false; continue; }
        if (line == "atoms:") { in_types = false; in_atoms = true; continue; }
        std::istringstream ls(line);
        std::vector<std::string> p;
        for (std::string t; ls >> t;) p.push_back(t);
        if (in_types && p.size() >= 2) {
            char *end = nullptr;
            float v = std::strtof(p[1].c_str(), &end);
            if (end && *end == '\0') types[p[0]] = v;
        } else if (in_atoms && p.size() >= 3) {
            auto t = types.find(p[2]);
            if (t != types.end()) atoms[p[0]][p[1]] = t->second;
        }
    }
    return atoms;
}

RadiiConfig load_radii_from_file(const std::string &path)
{
    std::ifstream f(path);
    if (!f) throw std::runtime_error("Failed to load radii file: " + path);
    std::stringstream ss;
    ss << f.rdbuf();
    return parse_radii_config(ss.str());
}

// Element van-der-Waals radii (Alvarez 2013, the table pdbtbx's
// Element::atomic_radius().van_der_waals is built from).  The reference's own
// tests pin N, C, O, S (tests/units.rs:18-43); the rest is unpinned here.
bool vdw_radius(const std::string &element, float *out)
{
    static const std::pair<const char *, float> t[] = {
        {"H", 1.20f},  {"HE", 1.43f}, {"LI", 2.12f}, {"BE", 1.98f}, {"B", 1.91f},  {"C", 1.77f},
        {"N", 1.66f},  {"O", 1.50f},  {"F", 1.46f},  {"NE", 1.58f}, {"NA", 2.50f}, {"MG", 2.51f},
        {"AL", 2.25f}, {"SI", 2.19f}, {"P", 1.90f},  {"S", 1.89f},  {"CL", 1.82f}, {"AR", 1.83f},
        {"K", 2.73f},  {"CA", 2.62f}, {"SC", 2.58f}, {"TI", 2.46f}, {"V", 2.42f},  {"CR", 2.45f},
        {"MN", 2.45f}, {"FE", 2.44f}, {"CO", 2.40f}, {"NI", 2.40f}, {"CU", 2.38f}, {"ZN", 2.39f},
        {"GA", 2.32f}, {"GE", 2.29f}, {"AS", 1.88f}, {"SE", 1.82f}, {"BR", 1.86f}, {"KR", 2.25f},
        {"RB", 3.21f}, {"SR", 2.84f}, {"MO", 2.45f}, {"CD", 2.49f}, {"I", 2.04f},  {"XE", 2.06f},
        {"CS", 3.48f}, {"BA", 3.03f}, {"W", 2.57f},  {"PT", 2.29f}, {"AU", 2.32f}, {"HG", 2.45f},
        {"PB", 2.60f}, {"U", 2.71f},  {"D", 1.20f}};
    for (const auto &e : t)
        if (element == e.first) { *out = e.second; return true; }
    return false;
}

}  // namespace rustsasa

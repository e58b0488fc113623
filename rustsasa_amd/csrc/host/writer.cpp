// Host API, part 3 of 5: output - the results as JSON in serde's shape, values written back into b-factors, the
// model as PDB text (reference src/utils/io.rs).
#include "host_internal.h"

#include <charconv>
#include <cmath>
#include <cstdio>
#include <fstream>

namespace rustsasa {

namespace {

void json_string(std::string &o, const std::string &s)
{
    o += '"';
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') { o += '\\'; o += (char)c; }
        else if (c < 0x20) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        else o += (char)c;
    }
    o += '"';
}

// shortest decimal that round-trips the f32, as serde_json (ryu) prints an f32: plain decimals with ".0" on whole numbers
// ("200.0", not "2e+02" - which round 5's %g search printed), an exponent without sign or padding outside [1e-5, 1e16)
// ("1e-7"), null for NaN and the infinities.  std::to_chars: 90 ns per value where the %.*g / strtof search took 2.4 us -
// directory mode with per-file JSON output prints a million and a half of them per proteome.
void json_f32(std::string &o, float v)
{
    if (!std::isfinite(v)) { o += "null"; return; }
    if (v == 0.0f) { o += std::signbit(v) ? "-0.0" : "0.0"; return; }
    char b[64];
    const auto r = std::to_chars(b, b + sizeof b, v, std::chars_format::scientific);  // shortest digits: [-]d[.ddd]e[+-]XX
    *r.ptr = 0;
    const char *p = b;
    if (*p == '-') { o += '-'; p++; }
    const char *e = std::strchr(p, 'e');
    char dig[16];
    int nd = 0;
    for (const char *q = p; q < e; q++)
        if (*q != '.') dig[nd++] = *q;
    const int ex = std::atoi(e + 1);
    if (ex < -5 || ex >= 16) {  // ryu's exponent form: "1e-7", "1.5e20"
        o += dig[0];
        if (nd > 1) { o += '.'; o.append(dig + 1, (size_t)nd - 1); }
        o += 'e';
        o += std::to_string(ex);
        return;
    }
    if (ex < 0) {
        o += "0.";
        o.append((size_t)(-ex - 1), '0');
        o.append(dig, (size_t)nd);
    } else if (ex >= nd - 1) {
        o.append(dig, (size_t)nd);
        o.append((size_t)(ex - (nd - 1)), '0');
        o += ".0";
    } else {
        o.append(dig, (size_t)ex + 1);
        o += '.';
        o.append(dig + ex + 1, (size_t)(nd - ex - 1));
    }
}

}  // namespace

std::string sasa_result_to_json(const std::vector<float> &v)
{
    std::string o = "{\"Atom\":[";
    for (size_t i = 0; i < v.size(); i++) { if (i) o += ','; json_f32(o, v[i]); }
    return o + "]}";
}

std::string sasa_result_to_json(const std::vector<ResidueResult> &v)
{
    std::string o = "{\"Residue\":[";
    for (size_t i = 0; i < v.size(); i++) {
        if (i) o += ',';
        o += "{\"serial_number\":" + std::to_string(v[i].serial_number) + ",\"insertion_code\":";
        json_string(o, v[i].insertion_code);
        o += ",\"value\":";
        json_f32(o, v[i].value);
        o += ",\"name\":";
        json_string(o, v[i].name);
        o += std::string(",\"is_polar\":") + (v[i].is_polar ? "true" : "false") + ",\"chain_id\":";
        json_string(o, v[i].chain_id);
        o += '}';
    }
    return o + "]}";
}

std::string sasa_result_to_json(const std::vector<ChainResult> &v)
{
    std::string o = "{\"Chain\":[";
    for (size_t i = 0; i < v.size(); i++) {
        if (i) o += ',';
        o += "{\"name\":";
        json_string(o, v[i].name);
        o += ",\"value\":";
        json_f32(o, v[i].value);
        o += '}';
    }
    return o + "]}";
}

std::string sasa_result_to_json(const ProteinResult &v)
{
    std::string o = "{\"Protein\":{\"global_total\":";
    json_f32(o, v.global_total);
    o += ",\"polar_total\":";
    json_f32(o, v.polar_total);
    o += ",\"non_polar_total\":";
    json_f32(o, v.non_polar_total);
    return o + "}}";
}

// io.rs:25-30: every atom of the model, in order, takes v[i]
bool sasa_result_to_protein_object(Structure &pdb, const std::vector<float> &v, std::string *err)
{
    if (pdb.atom_count() != v.size()) {
        if (err) *err = "atom-level result has " + std::to_string(v.size()) + " values for " +
                        std::to_string(pdb.atom_count()) + " atoms (filtered atoms cannot be mapped back)";
        return false;
    }
    size_t i = 0;
    for (auto &c : pdb.chains)
        for (auto &r : c.residues)
            for (auto &f : r.conformers)
                for (auto &a : f.atoms) a.b_factor = (double)v[i++];
    return true;
}

// io.rs:31-43
bool sasa_result_to_protein_object(Structure &pdb, const std::vector<ResidueResult> &v, std::string *err)
{
    size_t i = 0;
    for (auto &c : pdb.chains)
        for (auto &r : c.residues) {
            if (i >= v.size() || v[i].serial_number != r.serial_number) {
                if (err) *err = "residue-level result does not line up with the structure";
                return false;
            }
            for (auto &f : r.conformers)
                for (auto &a : f.atoms) a.b_factor = (double)v[i].value;
            i++;
        }
    return true;
}

// io.rs:44-54
bool sasa_result_to_protein_object(Structure &pdb, const std::vector<ChainResult> &v, std::string *err)
{
    if (v.size() != pdb.chains.size()) {
        if (err) *err = "chain-level result does not line up with the structure";
        return false;
    }
    for (size_t i = 0; i < pdb.chains.size(); i++) {
        if (v[i].name != pdb.chains[i].id) {
            if (err) *err = "chain-level result does not line up with the structure";
            return false;
        }
        for (auto &r : pdb.chains[i].residues)
            for (auto &f : r.conformers)
                for (auto &a : f.atoms) a.b_factor = (double)v[i].value;
    }
    return true;
}

// io.rs:55-61
bool sasa_result_to_protein_object(Structure &pdb, const ProteinResult &v, std::string *)
{
    for (auto &c : pdb.chains)
        for (auto &r : c.residues)
            for (auto &f : r.conformers)
                for (auto &a : f.atoms) a.b_factor = (double)v.global_total;
    return true;
}

std::string Structure::to_pdb_text() const
{
    std::string o;
    char line[96];
    for (const auto &c : chains) {
        for (const auto &r : c.residues)
            for (const auto &f : r.conformers)
                for (const auto &a : f.atoms) {
                    // atom names shorter than four characters start in column 14 unless the
                    // element symbol has two letters
                    std::string name = a.name;
                    if (name.size() < 4 && a.element.size() < 2) name = " " + name;
                    std::snprintf(line, sizeof line,
                                  "%-6s%5zu %-4s%1s%3s %1s%4lld%1s   %8.3f%8.3f%8.3f%6.2f%6.2f          %2s  \n",
                                  a.hetero ? "HETATM" : "ATOM", a.serial % 100000, name.c_str(),
                                  f.alt_loc.substr(0, 1).c_str(), f.name.substr(0, 3).c_str(),
                                  c.id.substr(0, 1).c_str(), (long long)(r.serial_number % 10000),
                                  r.insertion_code.substr(0, 1).c_str(), a.x, a.y, a.z, a.occupancy,
                                  a.b_factor, a.element.c_str());
                    o += line;
                }
        o += "TER\n";
    }
    o += "END\n";
    return o;
}

void Structure::save_pdb(const std::string &path) const
{
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write " + path);
    const std::string t = to_pdb_text();
    f.write(t.data(), (std::streamsize)t.size());
    if (!f) throw std::runtime_error("write failed: " + path);
}

}  // namespace rustsasa

// What the sub-commands of the `tetrex` command line share: the option parser and the clock.  main.cpp has query, index,
// track and inspect; search_cmd.cpp has search.
#pragma once
#include <chrono>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace tetrex {

inline double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Args {
    std::vector<std::string> pos;
    std::vector<std::pair<std::string, std::string>> opts;  // canonical long name -> value ("" for flags)
    bool has(const std::string& n) const {
        for (auto& o : opts) if (o.first == n) return true;
        return false;
    }
    std::string get(const std::string& n, const std::string& dflt) const {
        for (auto& o : opts) if (o.first == n) return o.second;
        return dflt;
    }
};

struct OptSpec { char s; const char* l; bool value; };

inline Args parse(int argc, char** argv, int from, const std::vector<OptSpec>& spec) {
    Args a;
    bool only_pos = false;
    for (int i = from; i < argc; ++i) {
        std::string t = argv[i];
        if (only_pos || t.size() < 2 || t[0] != '-' || t == "-") { a.pos.push_back(t); continue; }
        if (t == "--") { only_pos = true; continue; }
        const OptSpec* hit = nullptr;
        std::string inline_value;
        bool has_inline = false;
        if (t[1] == '-') {
            std::string name = t.substr(2);
            const size_t eq = name.find('=');
            if (eq != std::string::npos) { inline_value = name.substr(eq + 1); name = name.substr(0, eq); has_inline = true; }
            for (auto& s : spec) if (name == s.l) hit = &s;
        } else {
            for (auto& s : spec) if (t[1] == s.s) hit = &s;
            if (hit && t.size() > 2) {
                if (hit->value) { inline_value = t.substr(2); has_inline = true; }
                else {  // bundled flags: -vf
                    for (size_t j = 1; j < t.size(); ++j) {
                        const OptSpec* f = nullptr;
                        for (auto& s : spec) if (t[j] == s.s && !s.value) f = &s;
                        if (!f) throw std::runtime_error("Unknown option " + t);
                        a.opts.emplace_back(f->l, "");
                    }
                    continue;
                }
            }
        }
        if (!hit) throw std::runtime_error("Unknown option " + t);
        if (!hit->value) { a.opts.emplace_back(hit->l, ""); continue; }
        if (!has_inline) {
            if (i + 1 >= argc) throw std::runtime_error(std::string("Missing value for option --") + hit->l);
            inline_value = argv[++i];
        }
        a.opts.emplace_back(hit->l, inline_value);
    }
    return a;
}

// tetrex search ... (search_cmd.cpp)
int cmd_search(int argc, char** argv);

}  // namespace tetrex

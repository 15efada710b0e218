#include "validator.h"

#include <charconv>
#include <cmath>
#include <cstring>

namespace xgs {

std::string rust_f32_display(float v) {
  if (std::isnan(v)) return "NaN";
  if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
  char buf[128];
  // Shortest representation that round-trips, in fixed notation == Rust's
  // `impl Display for f32` (which never switches to exponent form).
  auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::fixed);
  std::string s(buf, r.ptr);
  if (s == "-0") return "-0";
  return s;
}

// Decode one code point; returns bytes consumed (>=1). Invalid sequences are
// consumed one byte at a time and treated as non-whitespace.
static size_t decode_utf8(const unsigned char* p, size_t n, uint32_t& cp) {
  unsigned char c = p[0];
  if (c < 0x80) { cp = c; return 1; }
  size_t len = (c >> 5) == 0x6 ? 2 : (c >> 4) == 0xE ? 3 : (c >> 3) == 0x1E ? 4 : 0;
  if (len == 0 || len > n) { cp = 0xFFFD; return 1; }
  cp = c & (0xFF >> (len + 1));
  for (size_t i = 1; i < len; ++i) {
    if ((p[i] & 0xC0) != 0x80) { cp = 0xFFFD; return 1; }
    cp = (cp << 6) | (p[i] & 0x3F);
  }
  return len;
}

// Unicode White_Space property (what Rust's char::is_whitespace tests).
static bool is_unicode_ws(uint32_t c) {
  if (c >= 0x09 && c <= 0x0D) return true;
  switch (c) {
    case 0x20: case 0x85: case 0xA0: case 0x1680: case 0x2028: case 0x2029:
    case 0x202F: case 0x205F: case 0x3000:
      return true;
    default:
      return c >= 0x2000 && c <= 0x200A;
  }
}

bool is_blank_utf8(const std::string& s) {
  const unsigned char* p = reinterpret_cast<const unsigned char*>(s.data());
  size_t n = s.size(), i = 0;
  while (i < n) {
    uint32_t cp;
    size_t k = decode_utf8(p + i, n - i, cp);
    if (!is_unicode_ws(cp)) return false;
    i += k;
  }
  return true;
}

static ValidationResult empty_prompt() {
  ValidationResult r;
  r.kind = ValidationKind::EmptyPrompt;
  r.message = "Empty prompt not allowed";
  return r;
}

static ValidationResult missing(const std::string& f) {
  ValidationResult r;
  r.kind = ValidationKind::MissingField;
  r.field = f;
  r.message = "Missing required field: " + f;
  return r;
}

static ValidationResult token_limit(size_t actual, size_t limit) {
  ValidationResult r;
  r.kind = ValidationKind::TokenLimitExceeded;
  r.actual = actual;
  r.limit = limit;
  r.message = "Token limit exceeded: " + std::to_string(actual) + " tokens > " +
              std::to_string(limit) + " max";
  return r;
}

static ValidationResult invalid_param(const std::string& f, const std::string& reason) {
  ValidationResult r;
  r.kind = ValidationKind::InvalidParameter;
  r.field = f;
  r.reason = reason;
  r.message = "Invalid parameter '" + f + "': " + reason;
  return r;
}

ValidationResult RequestValidator::check_sampling(size_t max_tokens, float temperature,
                                                  float top_p) const {
  if (max_tokens > cfg_.max_output_tokens)
    return invalid_param("max_tokens", "must be <= " + std::to_string(cfg_.max_output_tokens) +
                                           ", got " + std::to_string(max_tokens));
  bool t_bad = temperature < cfg_.min_temperature || temperature > cfg_.max_temperature ||
               (cfg_.reject_nan && std::isnan(temperature));
  if (t_bad)
    return invalid_param("temperature", "must be between " + rust_f32_display(cfg_.min_temperature) +
                                            " and " + rust_f32_display(cfg_.max_temperature) +
                                            ", got " + rust_f32_display(temperature));
  bool p_bad = top_p < cfg_.min_top_p || top_p > cfg_.max_top_p ||
               (cfg_.reject_nan && std::isnan(top_p));
  if (p_bad)
    return invalid_param("top_p", "must be between " + rust_f32_display(cfg_.min_top_p) + " and " +
                                      rust_f32_display(cfg_.max_top_p) + ", got " +
                                      rust_f32_display(top_p));
  return ValidationResult{};
}

static bool outside(float v, float lo, float hi) { return std::isnan(v) || v < lo || v > hi; }

ValidationResult RequestValidator::check_processors(float min_p, float repetition_penalty,
                                                    float presence_penalty, float frequency_penalty,
                                                    const std::vector<uint64_t>& bias_ids,
                                                    const std::vector<float>& bias_values,
                                                    uint64_t vocab_size) const {
  if (outside(min_p, 0.0f, 1.0f))
    return invalid_param("min_p", "must be between 0 and 1, got " + rust_f32_display(min_p));
  if (outside(repetition_penalty, 0.0f, 2.0f) || repetition_penalty == 0.0f)
    return invalid_param("repetition_penalty", "must be greater than 0 and at most 2, got " +
                                                   rust_f32_display(repetition_penalty));
  if (outside(presence_penalty, -2.0f, 2.0f))
    return invalid_param("presence_penalty",
                         "must be between -2 and 2, got " + rust_f32_display(presence_penalty));
  if (outside(frequency_penalty, -2.0f, 2.0f))
    return invalid_param("frequency_penalty",
                         "must be between -2 and 2, got " + rust_f32_display(frequency_penalty));
  if (bias_ids.size() != bias_values.size())
    return invalid_param("logit_bias", "token ids and values differ in number");
  if (bias_ids.size() > kMaxLogitBias)
    return invalid_param("logit_bias", "must have at most " + std::to_string(kMaxLogitBias) +
                                           " entries, got " + std::to_string(bias_ids.size()));
  for (size_t i = 0; i < bias_ids.size(); ++i) {
    if (vocab_size != 0 && bias_ids[i] >= vocab_size)
      return invalid_param("logit_bias", "token id " + std::to_string(bias_ids[i]) +
                                             " is outside the vocabulary of " + std::to_string(vocab_size));
    for (size_t j = 0; j < i; ++j)
      if (bias_ids[j] == bias_ids[i])
        return invalid_param("logit_bias", "token id " + std::to_string(bias_ids[i]) + " is given twice");
    if (outside(bias_values[i], -100.0f, 100.0f))
      return invalid_param("logit_bias", "bias of token " + std::to_string(bias_ids[i]) +
                                             " must be between -100 and 100, got " +
                                             rust_f32_display(bias_values[i]));
  }
  return ValidationResult{};
}

ValidationResult RequestValidator::check_top_logprobs(long long n) const {
  if (n < 0 || n > kMaxTopLogprobs)
    return invalid_param("top_logprobs", "must be an integer between 0 and " +
                                             std::to_string(kMaxTopLogprobs) + ", got " + std::to_string(n));
  return ValidationResult{};
}

ValidationResult RequestValidator::validate_generate(const std::string& prompt, size_t max_tokens,
                                                     float temperature, float top_p) const {
  if (is_blank_utf8(prompt)) return empty_prompt();
  size_t n = token_count(prompt);
  if (n > cfg_.max_context_tokens) return token_limit(n, cfg_.max_context_tokens);
  return check_sampling(max_tokens, temperature, top_p);
}

ValidationResult RequestValidator::validate_chat(const std::vector<std::string>& contents,
                                                 size_t max_tokens, float temperature,
                                                 float top_p) const {
  if (contents.empty()) return missing("messages");
  bool has = false;
  for (const auto& c : contents)
    if (!is_blank_utf8(c)) { has = true; break; }
  if (!has) return empty_prompt();
  size_t total = 0;
  for (const auto& c : contents) total += token_count(c);
  if (total > cfg_.max_context_tokens) return token_limit(total, cfg_.max_context_tokens);
  return check_sampling(max_tokens, temperature, top_p);
}

ValidationResult RequestValidator::validate_embeddings(const std::vector<std::string>& inputs) const {
  if (inputs.empty()) return missing("input");
  for (size_t i = 0; i < inputs.size(); ++i) {
    if (is_blank_utf8(inputs[i]))
      return invalid_param("input[" + std::to_string(i) + "]", "cannot be empty");
    size_t n = token_count(inputs[i]);
    if (n > cfg_.max_context_tokens) return token_limit(n, cfg_.max_context_tokens);
  }
  return ValidationResult{};
}

}  // namespace xgs

// Stand-in for <spdlog/spdlog.h> (TEST INFRASTRUCTURE): rebvio/util/log.hpp only needs the logger type to exist; the
// hot-path sources log nothing through it.
#ifndef REBVIO_REF_SHIM_SPDLOG_H_
#define REBVIO_REF_SHIM_SPDLOG_H_
namespace spdlog {
class logger {
 public:
  template <class... A> void trace(const A&...) {}
  template <class... A> void debug(const A&...) {}
  template <class... A> void info(const A&...) {}
  template <class... A> void warn(const A&...) {}
  template <class... A> void error(const A&...) {}
  template <class... A> void critical(const A&...) {}
};
}  // namespace spdlog
#endif

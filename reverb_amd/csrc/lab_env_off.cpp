// librvb.so only: the product library reads no tuning switch from the environment, every one takes its default (common.h lab_env).
// librvb_test.so links test_api.hip's getenv form instead.
namespace rvb {
const char* lab_env(const char*) { return nullptr; }
}

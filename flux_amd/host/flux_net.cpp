// flux_net.cpp -- see flux_net.hpp.
#include <algorithm>
#include "flux_net.hpp"
#include "scene_schema.hpp"

#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <unistd.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace flux_host {

using cbor::Decoder;
using cbor::Encoder;
using cbor::Type;

// =================================================================================================
// message codecs: the field and variant lists of scene_schema.hpp, walked by one CBOR writer and one CBOR reader
// =================================================================================================
template <class V> void variants(V &v, NetworkWorkerRequest &r) {  // workers.rs:105-110
    auto variant = [&](const char *name, NetworkWorkerRequest::Kind kind, auto &payload) {
        v.variant(name, r.kind == kind, [&]() -> decltype(payload) { r.kind = kind; return payload; });
    };
    variant("SetJob", NetworkWorkerRequest::SetJob, r.job);
    variant("WorkUnit", NetworkWorkerRequest::WorkUnitMsg, r.unit);
    v.unit_variant("Done", r.kind == NetworkWorkerRequest::Done, [&] { r.kind = NetworkWorkerRequest::Done; });
}

namespace {

// serde derive layouts; enums in serde_cbor <= 0.9's array form (cbor.hpp).  The lists take non-const references, so the
// encode_* functions cast const away for this visitor, which only reads.
struct CborWriter {
    Encoder &e;

    template <class M> void operator()(const char *name, M &member) {
        e.key(name);
        value(member);
    }
    template <class Select> void variant(const char *name, bool active, Select select) {
        if (!active) return;
        e.array(2);
        e.text(name);
        value(select());
    }
    template <class Select> void unit_variant(const char *name, bool active, Select) {
        if (active) e.text(name);
    }

    void value(double &v) { e.real(v); }
    void value(size_t &v) { e.uint(v); }
    void value(bool &v) { e.boolean(v); }
    void value(std::string &s) { e.text(s); }
    void value(Vec3 &v) {  // nalgebra Point3 / Vector3: a 3-sequence
        e.array(3);
        e.real(v.x);
        e.real(v.y);
        e.real(v.z);
    }
    void value(JobID &id) {  // tuple struct JobID(usize, usize), job.rs:12
        e.array(2);
        e.uint(id.allocator_id);
        e.uint(id.id);
    }
    void value(SystemTime &t) {
        const double secs = std::floor(t.seconds);
        SystemTimeParts p{secs < 0 ? 0 : (size_t)secs, (size_t)((t.seconds - secs) * 1e9)};
        if (p.nanos_since_epoch > 999999999ull) p.nanos_since_epoch = 999999999ull;
        value(p);
    }
    template <class T> void value(std::vector<T> &items) {
        e.array(items.size());
        for (T &item : items) value(item);
    }
    void value(MaterialData &m) { enumeration(m); }
    void value(ShapeData &s) { enumeration(s); }
    template <class E> void enumeration(E &en) { variants(*this, en); }  // the active variant writes itself
    template <class S> void value(S &s) {  // a struct: a map keyed by field name
        e.map(field_count(s));
        fields(*this, s);
    }
};

// Tolerant as cbor.hpp describes: maps in any key order, unknown keys skipped (serde ignores them), an absent key leaves the
// field's default, enums in all three layouts, definite and indefinite lengths.
struct CborReader {
    Decoder &d;

    bool value(double &v) { return d.read_number(v); }
    bool value(size_t &v) {
        uint64_t u;
        if (!d.read_uint(u)) return false;
        v = (size_t)u;
        return true;
    }
    bool value(bool &v) { return d.read_bool(v); }
    bool value(std::string &s) { return d.read_text(s); }
    // 3 numbers as a sequence (nalgebra; colours written as sequences) -- or the struct's map
    template <class T> bool triple(T &t, double &a, double &b, double &c) {
        if (d.peek() != Type::Array) return structure(t);
        uint64_t n;
        if (!d.read_array(n)) return false;
        if (!d.read_number(a) || !d.read_number(b) || !d.read_number(c)) return false;
        if (n == Decoder::kIndefinite) return d.at_break();
        return n == 3;
    }
    bool value(Vec3 &v) { return triple(v, v.x, v.y, v.z); }
    bool value(Color &c) { return triple(c, c.r, c.g, c.b); }
    bool value(JobID &id) {
        uint64_t n;
        if (!d.read_array(n) || !value(id.allocator_id) || !value(id.id)) return false;
        if (n == Decoder::kIndefinite) return d.at_break();
        return n == 2;
    }
    bool value(SystemTime &t) {
        SystemTimeParts p;
        if (!structure(p)) return false;
        t.seconds = (double)p.secs_since_epoch + (double)p.nanos_since_epoch * 1e-9;
        return true;
    }
    template <class T> bool sequence(std::vector<T> &items, uint64_t reserve_cap) {
        uint64_t n;
        if (!d.read_array(n)) return false;
        items.clear();
        if (n != Decoder::kIndefinite) items.reserve((size_t)std::min(n, reserve_cap));
        for (uint64_t i = 0; n == Decoder::kIndefinite ? !d.at_break() : i < n; i++) {
            T item;
            if (d.failed() || !value(item)) return false;
            items.push_back(std::move(item));
        }
        return !d.failed();
    }
    template <class T> bool value(std::vector<T> &items) { return sequence(items, 0); }
    bool value(std::vector<Color> &row) { return sequence(row, 1u << 16); }  // a frame row; the count is peer-controlled
    bool value(MaterialData &m) { return enumeration(m); }
    bool value(ShapeData &s) { return enumeration(s); }
    template <class S> bool value(S &s) { return structure(s); }

    // the field called `key`, if the struct has one, reads its value
    struct Field {
        CborReader &r;
        const std::string &key;
        bool found = false, ok = false;
        template <class M> void operator()(const char *name, M &member) {
            if (found || key != name) return;
            found = true;
            ok = r.value(member);
        }
    };
    template <class S> bool structure(S &s) {
        uint64_t n;
        if (!d.read_map(n)) return false;
        std::string key;
        for (uint64_t k = 0; n == Decoder::kIndefinite ? !d.at_break() : k < n; k++) {
            if (d.failed() || !d.read_text(key)) return false;
            Field field{*this, key};
            fields(field, s);
            if (field.found ? !field.ok : !d.skip()) return false;
        }
        return !d.failed();
    }

    // the variant called `name`, if the enum has one, becomes current and reads its payload
    struct Variant {
        CborReader &r;
        const std::string &name;
        bool has_payload, ok = false;
        template <class Select> void variant(const char *n, bool, Select select) {
            if (name == n) ok = has_payload && r.value(select());
        }
        template <class Select> void unit_variant(const char *n, bool, Select select) {
            if (name != n || has_payload) return;
            select();
            ok = true;
        }
    };
    // "Name" | [name, payload, ..] (serde_cbor <= 0.9) | {name: payload} (>= 0.10); false on an unknown variant
    template <class E> bool enumeration(E &en) {
        std::string name;
        auto payload = [&](bool has) {
            Variant chosen{*this, name, has};
            variants(chosen, en);
            return chosen.ok;
        };
        const Type t = d.peek();
        uint64_t n;
        if (t == Type::Text) return d.read_text(name) && payload(false);
        if (t == Type::Array) {
            if (!d.read_array(n) || !d.read_text(name)) return false;
            if (n == 1) return payload(false);
            if (!payload(true)) return false;
            if (n == Decoder::kIndefinite) {
                while (!d.at_break())
                    if (d.failed() || !d.skip()) return false;
            } else {
                for (uint64_t k = 2; k < n; k++)
                    if (!d.skip()) return false;
            }
            return !d.failed();
        }
        if (t == Type::Map) {
            if (!d.read_map(n) || !d.read_text(name) || !payload(true)) return false;
            if (n == Decoder::kIndefinite) return d.at_break();
            return n == 1;
        }
        return false;
    }
};

}  // namespace

void encode_worker_info(Encoder &e, const WorkerInfo &w) { CborWriter{e}.value(const_cast<WorkerInfo &>(w)); }
void encode_request(Encoder &e, const NetworkWorkerRequest &r) { CborWriter{e}.enumeration(const_cast<NetworkWorkerRequest &>(r)); }
void encode_event(Encoder &e, const RenderEvent &ev) { CborWriter{e}.enumeration(const_cast<RenderEvent &>(ev)); }
bool decode_worker_info(Decoder &d, WorkerInfo &w) { return CborReader{d}.structure(w); }
bool decode_request(Decoder &d, NetworkWorkerRequest &r) { return CborReader{d}.enumeration(r); }
bool decode_event(Decoder &d, RenderEvent &ev) { return CborReader{d}.enumeration(ev); }

// =================================================================================================
// TCP
// =================================================================================================
TcpStream::~TcpStream() {
    if (fd_ >= 0) ::close(fd_);
}

bool TcpStream::read(void *dst, size_t n) {
    char *p = static_cast<char *>(dst);
    while (n > 0) {
        const ssize_t got = ::recv(fd_, p, n, 0);
        if (got > 0) {
            p += got;
            n -= (size_t)got;
        } else if (got < 0 && errno == EINTR) {
            continue;
        } else {
            return false;
        }
    }
    return true;
}

bool TcpStream::write_all(const std::string &bytes) {
    const char *p = bytes.data();
    size_t n = bytes.size();
    while (n > 0) {
        const ssize_t put = ::send(fd_, p, n, MSG_NOSIGNAL);
        if (put > 0) {
            p += put;
            n -= (size_t)put;
        } else if (put < 0 && errno == EINTR) {
            continue;
        } else {
            return false;
        }
    }
    return true;
}

void TcpStream::shutdown_both() {
    if (fd_ >= 0) ::shutdown(fd_, SHUT_RDWR);
}

std::string TcpStream::peer() const {
    sockaddr_storage ss;
    socklen_t len = sizeof ss;
    char host[NI_MAXHOST] = "?", serv[NI_MAXSERV] = "?";
    if (::getpeername(fd_, (sockaddr *)&ss, &len) == 0)
        ::getnameinfo((sockaddr *)&ss, len, host, sizeof host, serv, sizeof serv, NI_NUMERICHOST | NI_NUMERICSERV);
    return std::string(host) + ":" + serv;
}

static void split_endpoint(const std::string &raw, std::string &host, std::string &port) {
    const size_t colon = raw.find(':');  // workers.rs:120-123: no ':' -> default port
    if (colon == std::string::npos) {
        host = raw;
        port = kDefaultPort;
    } else {
        host = raw.substr(0, colon);
        port = raw.substr(colon + 1);
    }
}

std::unique_ptr<TcpStream> TcpStream::connect(const std::string &endpoint) {
    std::string host, port;
    split_endpoint(endpoint, host, port);
    addrinfo hints{}, *res = nullptr;
    hints.ai_family = AF_UNSPEC;
    hints.ai_socktype = SOCK_STREAM;
    const int rc = ::getaddrinfo(host.c_str(), port.c_str(), &hints, &res);
    if (rc != 0) throw FluxError(FLUX_E_IO, "cannot resolve " + endpoint + ": " + gai_strerror(rc));
    int fd = -1;
    std::string last = "no address";
    for (addrinfo *a = res; a; a = a->ai_next) {
        fd = ::socket(a->ai_family, a->ai_socktype, a->ai_protocol);
        if (fd < 0) continue;
        if (::connect(fd, a->ai_addr, a->ai_addrlen) == 0) break;
        last = std::strerror(errno);
        ::close(fd);
        fd = -1;
    }
    ::freeaddrinfo(res);
    if (fd < 0) throw FluxError(FLUX_E_IO, "cannot connect to " + endpoint + ": " + last);
    int one = 1;
    ::setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
    return std::unique_ptr<TcpStream>(new TcpStream(fd));
}

// =================================================================================================
// NodeServer: flux-node/src/main.rs:21-111
// =================================================================================================
NodeServer::NodeServer(const std::string &host, const std::string &port, WorkerHandle worker, size_t num_threads)
    : worker_(std::move(worker)), num_threads_(num_threads) {
    addrinfo hints{}, *res = nullptr;
    hints.ai_family = AF_INET;
    hints.ai_socktype = SOCK_STREAM;
    hints.ai_flags = AI_PASSIVE;
    const int rc = ::getaddrinfo(host.c_str(), port.c_str(), &hints, &res);
    if (rc != 0) throw FluxError(FLUX_E_IO, "cannot resolve bind address " + host + ":" + port + ": " + gai_strerror(rc));
    const int fd = ::socket(res->ai_family, res->ai_socktype, res->ai_protocol);
    int one = 1;
    if (fd >= 0) ::setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one);
    if (fd < 0 || ::bind(fd, res->ai_addr, res->ai_addrlen) != 0 || ::listen(fd, 4) != 0) {
        const std::string why = std::strerror(errno);
        ::freeaddrinfo(res);
        if (fd >= 0) ::close(fd);
        throw FluxError(FLUX_E_IO, "cannot listen on " + host + ":" + port + ": " + why);
    }
    ::freeaddrinfo(res);
    sockaddr_in sa{};
    socklen_t len = sizeof sa;
    if (::getsockname(fd, (sockaddr *)&sa, &len) == 0) port_ = ntohs(sa.sin_port);
    listen_fd_ = fd;
}

NodeServer::~NodeServer() { stop(); }

void NodeServer::stop() {
    stopping_ = true;
    const int fd = listen_fd_.exchange(-1);
    if (fd >= 0) {
        ::shutdown(fd, SHUT_RDWR);
        ::close(fd);
    }
}

void NodeServer::serve_forever() {  // run_server: one client at a time (main.rs:100-108)
    while (!stopping_) {
        const int lfd = listen_fd_.load();
        if (lfd < 0) break;
        const int fd = ::accept(lfd, nullptr, nullptr);
        if (fd < 0) {
            if (stopping_) break;
            if (errno == EINTR) continue;
            break;
        }
        int one = 1;
        ::setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
        if (!handle_client(std::unique_ptr<TcpStream>(new TcpStream(fd))))
            std::printf("run_server: handle_client exited with an error\n");
        clients_++;
    }
}

bool NodeServer::handle_client(std::unique_ptr<TcpStream> stream) {
    std::printf("Got connection from %s\n", stream->peer().c_str());
    {
        Encoder e;  // main.rs:26-31
        encode_worker_info(e, WorkerInfo{num_threads_});
        if (!stream->write_all(e.out)) return false;
    }
    auto wu = std::make_shared<Channel<WorkUnit>>();
    auto re = std::make_shared<Channel<std::optional<RenderEvent>>>();
    auto wg = std::make_shared<WaitGroup>();
    TcpStream *raw = stream.get();
    JoiningThread writer;
    // The reference returns right away and lets the channel drops end the worker's job; here, on every path out of this function,
    // the unit channel is closed, the worker finishes the units it already holds, its last events are flushed and the writer is
    // woken; then the writer is joined.
    ScopeExit release{[&] {
        wu->close();
        wg->wait();
        re->send(std::nullopt);
    }};
    // result writer (main.rs:41-55): every RenderEvent of the local worker goes back to the manager
    writer = JoiningThread([raw, re] {
        while (auto m = re->recv()) {
            if (!*m) break;
            Encoder e;
            encode_event(e, **m);
            if (!raw->write_all(e.out)) {
                std::printf("Manager connection error\n");
                return;
            }
        }
    });
    Decoder dec(*stream);
    for (;;) {  // for result in stream_de (main.rs:57-87)
        if (dec.peek() == Type::End) break;  // the client closed the stream
        NetworkWorkerRequest req;
        if (!decode_request(dec, req)) {
            std::printf("handle_client: bad request: %s\n", dec.error().empty() ? "unexpected message" : dec.error().c_str());
            return false;
        }
        if (req.kind == NetworkWorkerRequest::SetJob) {
            std::printf("Got job\n");
            worker_.send(std::make_shared<Job>(std::move(req.job)), wu, re, wg);
        } else if (req.kind == NetworkWorkerRequest::WorkUnitMsg) {
            wu->send(req.unit);
        } else {
            std::printf("Got done message, shutting down\n");
            break;
        }
    }
    return true;
}

// =================================================================================================
// NetworkWorker: workers.rs:112-258
// =================================================================================================
static WorkerInfo node_info(TcpStream &stream, const std::string &raw_endpoint) {
    std::printf("Getting info\n");
    Decoder d(stream);  // the first message is the node's WorkerInfo (workers.rs:134-141)
    WorkerInfo info;
    if (!decode_worker_info(d, info)) throw FluxError(FLUX_E_IO, "Could not get info from network node " + raw_endpoint);
    std::printf("Got info\n");
    return info;
}

NetworkWorker::NetworkWorker(const std::string &raw_endpoint)
    : stream_(TcpStream::connect(raw_endpoint)), info_(node_info(*stream_, raw_endpoint)), service_([this] { run(); }) {}

void NetworkWorker::run() {
    Decoder events(*stream_);
    auto send_request = [&](const NetworkWorkerRequest &r) {
        Encoder e;
        encode_request(e, r);
        return stream_->write_all(e.out);
    };
    // forwards one RenderEvent from the node; false when the stream ended or broke
    auto forward_one = [&](const std::shared_ptr<Channel<std::optional<RenderEvent>>> &out) {
        RenderEvent ev;
        if (events.peek() == Type::End || !decode_event(events, ev)) return false;
        out->send(std::move(ev));
        return true;
    };
    for (;;) {  // while let Ok(Some((job, recv_unit, send_result, wg))) = r.recv()   (workers.rs:152)
        auto msg = service_.next();
        if (!msg) break;
        const WorkerRequest req = std::move(*msg);  // dropped at the end of the pass: drop(wg)
        bool alive = true;
        NetworkWorkerRequest set;
        set.kind = NetworkWorkerRequest::SetJob;
        set.job = *req.job;
        alive = send_request(set);  // workers.rs:159
        size_t sent = 0;
        for (int k = 0; alive && k < 2; k++) {  // two units in flight (workers.rs:161-175)
            auto unit = req.recv_unit->recv();
            if (!unit) break;
            NetworkWorkerRequest r;
            r.kind = NetworkWorkerRequest::WorkUnitMsg;
            r.unit = *unit;
            alive = send_request(r);
            sent++;
        }
        while (alive) {  // one out, one in (workers.rs:179-201)
            auto unit = req.recv_unit->recv();
            if (!unit) break;
            NetworkWorkerRequest r;
            r.kind = NetworkWorkerRequest::WorkUnitMsg;
            r.unit = *unit;
            alive = send_request(r) && forward_one(req.send_result);
        }
        for (size_t k = 0; alive && k < sent; k++) alive = forward_one(req.send_result);  // workers.rs:205-222
        if (alive) {
            NetworkWorkerRequest done;
            done.kind = NetworkWorkerRequest::Done;  // workers.rs:226
            alive = send_request(done);
        }
        if (!alive) {
            std::fprintf(stderr, "NetworkWorker: connection to the node lost\n");
            break;  // the reference's thread returns on a deserializer error (workers.rs:194-197)
        }
    }
}

}  // namespace flux_host
